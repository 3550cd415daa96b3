"""The KITTI object benchmark's own protocol on Omni3D records: AP|R40 (and AP|R11) of the 2D box, the bird's-eye view and the 3D box
at Easy / Moderate / Hard, per class (`KittiEval`, csrc/eval_kitti.hip).  The reference has no counterpart.

The protocol is a READING of the devkit's `evaluate_object` written down from memory -- the devkit is not part of this repository --
and stated in float64 by tests/exact_kitti.py.  It is a different pipeline from `Omni3Deval` (which matches detections to ground truths
COCO-style and accumulates over a recall axis) and therefore not a `Mode` of modes.py:

  * ground truths are walked, not detections; one greedy pass harvests the scores of the true positives, up to 41 score thresholds are
    derived from them, and another greedy pass runs per threshold;
  * difficulty is (min 2D box height, max occlusion, max truncation); a ground truth of the class outside the difficulty, and every
    ground truth of a neighbour class (van for car, person for pedestrian), is neutral: a detection on it counts for nothing;
  * DontCare regions absorb false positives (in the metrics of `dcMetrics`) by intersection / area of the detection's 2D box;
  * min-overlaps are per class and strict (`>`), compared as doubles.

Precision is indexed by THRESHOLD as in the devkit, so a slot with fewer than 80 counted ground truths cannot reach 100 (20 ground truths,
all found, give 47.5).  That is the benchmark's behaviour and is kept.

Departures and conventions ("KITTI-protocol evaluation"): the 2D box is the `bbox` the Omni3D index selects (the projected
cuboid, or KITTI's own hand-drawn box with MODAL_2D_BOXES), the occlusion level comes from `visibility` through `occCuts` unless an
annotation carries an integer `occlusion`, BEV and 3D overlaps are the project's footprint IoU (`kernels.bev`) and exact cuboid IoU
(`kernels.iou3d.iou_box3d_exact_pairs`), which equal KITTI's rotated-box IoUs for yaw-only boxes.

AOS (`KittiParams.aos`, off by default): the benchmark's average orientation similarity of the 2D-box matching, again a reading of the
devkit (its `compute_aos` path) written from memory; float64 statement: tests/exact_kitti_aos.py.  Every true positive of pass 2 adds
(1 + cos(alpha_gt - alpha_dt)) / 2, the sum is divided by tp + fp and treated like precision.  The observation angle alpha of a record
is its own finite `alpha` key (KITTI's "unknown" -10 counts as absent), else it comes from the cuboid's corners
(`kernels.kitti.box_params`: the corner order makes v1 - v0 the length axis, whose angle in the ground plane is KITTI's rotation_y);
a record with neither has no heading and contributes 0.  Label files: `cubercnn.data.kitti_format`."""
import json

import numpy as np
import torch

from ...kernels import bev, iou3d
from ...kernels import kitti as K
from .pairs import _pairs_pass, _ragged_pairs, _xywh_iou

METRIC_NAMES = {"2D": ("bbox", "AP2D"), "BEV": ("bev", "APBEV"), "3D": ("3d", "AP3D")}


class KittiParams:
    """The protocol's tables, overridable like `Omni3DParams` (set attributes before `evaluate()`).

    occCuts: occlusion level = the number of cuts c with visibility <= c (0 for an unknown, negative visibility).  The cuts are a
    CONVENTION of this project; they have not been checked against the converter that made Omni3D's KITTI annotations.
    dcMetrics: the metrics in which DontCare regions absorb false positives; all three is this project's reading of the C++ devkit
    (its numba port restricts the step to 2D).
    aos: also compute the average orientation similarity of the 2D-box matching (it needs "2D" among `metrics`, as in the devkit)."""

    def __init__(self):
        self.aos = False
        self.classes = ("car", "pedestrian", "cyclist")
        self.minOverlaps = {"strict": (0.7, 0.5, 0.5), "loose": (0.5, 0.25, 0.25)}
        self.neighbours = {"car": ("van",), "pedestrian": ("person",)}
        self.dontcareNames = ("dontcare",)
        self.difficulties = [("easy", 40, 0, 0.15), ("moderate", 25, 1, 0.30), ("hard", 25, 2, 0.50)]
        self.metrics = ("2D", "BEV", "3D")
        self.dcMetrics = ("2D", "BEV", "3D")
        self.occCuts = (0.75, 0.5, 0.25)
        self.nSamplePts = 41
        self.up = (0.0, -1.0, 0.0)

    def check(self):
        if any(m not in METRIC_NAMES for m in tuple(self.metrics) + tuple(self.dcMetrics)):
            raise ValueError("metrics / dcMetrics must be taken from %s" % (tuple(METRIC_NAMES),))
        if any(len(v) != len(self.classes) for v in self.minOverlaps.values()):
            raise ValueError("every set of minOverlaps needs one value per class")
        if any(not float(x) >= 0 for v in self.minOverlaps.values() for x in v):
            raise ValueError("min-overlaps must be >= 0")
        if not 2 <= int(self.nSamplePts) <= K.MAX_PTS:
            raise ValueError("nSamplePts must lie in [2, %d]" % K.MAX_PTS)
        if any(len(d) != 4 for d in self.difficulties):
            raise ValueError("a difficulty is (name, min height, max occlusion, max truncation)")
        if self.aos and "2D" not in self.metrics:
            raise ValueError("aos belongs to the matching of the 2D box: metrics must contain \"2D\"")


def record_alpha(a):
    """the observation angle a record states itself: its finite `alpha` key, KITTI's "unknown" -10 counting as absent -> float or NaN"""
    v = a.get("alpha")
    if v is None:
        return float("nan")
    v = float(v)
    return v if np.isfinite(v) and v != -10.0 else float("nan")


def occlusion_level(ann, cuts):
    if ann.get("occlusion") is not None:
        return int(ann["occlusion"])
    v = float(ann.get("visibility", -1))
    return 0 if v < 0 else sum(1 for c in cuts if v <= c)


_NAN_BOX = [[float("nan")] * 3] * 8


def _gt_records(gt, names):
    """-> (image ids in order, {image id: [annotation dicts]}, name of an annotation, the category names the data set knows)"""
    known = set()
    if isinstance(gt, (list, tuple)):                      # dataset dicts: {'image_id', 'annotations': [...]}
        img_ids = [d["image_id"] for d in gt]
        by_img = {d["image_id"]: list(d.get("annotations", [])) for d in gt}
        cats = {}
    else:
        cats = {i: c["name"] for i, c in getattr(gt, "cats", {}).items()}
        if hasattr(gt, "imgToAnns") and hasattr(gt, "imgs"):
            img_ids = sorted(gt.imgs.keys())
            by_img = {i: list(gt.imgToAnns.get(i, [])) for i in img_ids}
        else:                                              # AnnotationIndex
            img_ids = sorted(gt.getImgIds())
            by_img = {i: [] for i in img_ids}
            for a in gt.loadAnns(gt.getAnnIds(imgIds=img_ids)):
                by_img.setdefault(a["image_id"], []).append(a)
    if names is not None:
        cats.update(dict(enumerate(names)) if isinstance(names, (list, tuple)) else names)
    known.update(str(n).lower() for n in cats.values())

    def name_of(a):
        n = a.get("category_name")
        if n is None:
            n = cats.get(a.get("category_id"))
        return None if n is None else str(n).lower()

    known.update(n for anns in by_img.values() for n in (name_of(a) for a in anns) if n is not None)
    return img_ids, by_img, name_of, known


class KittiEval:
    """`KittiEval(gt, dt, names=None)`: evaluate() -> summarize().

    gt: the `Omni3D` index (filter settings applied, so every annotation has `bbox`, `bbox3D` and the ignore flags), an
    `AnnotationIndex`, or a list of dataset dicts ({'image_id', 'annotations'}).  dt: the records of `omni_instances_results.json`
    (`image_id`, `category_id`, `score`, `bbox` XYWH, `bbox3D` 8 x 3) as a list, a path, or an index with `loadAnns`.  names: category
    id -> name (a dict, or a list indexed by id) where the records carry no `category_name` and `gt` has no category table.  img_ids:
    None, or the images to evaluate (the others, and their detections, take no part).

    Per ground truth: height = h of `bbox`; truncation, 0 when negative (unknown); occlusion = `occlusion_level`.  A ground truth named
    in `dontcareNames` is a DontCare region (its 2D box only).  A ground truth of the class whose `ignore` / `ignore2D` / `ignore3D` is
    set is neutral where the difficulty's three bounds exclude it anyway and NO candidate (flag -1: it is not counted and absorbs
    nothing) where they would count it: the flag was set for a reason the protocol does not know (no valid 3D box, no lidar support, a
    depth or height filter), and guessing that such an object is detectable is not this evaluator's call.  A ground truth without a
    valid 3D box has BEV and 3D overlap 0 with everything.

    `eval` after evaluate(): `precision`, `recall`, `thresholds` [class, difficulty, metric, overlap set, 41], `counts` [..., 41, 3]
    (tp, fp, fn), `n_gt`, `K`, `ap_r40`, `ap_r11` [class, difficulty, metric, overlap set]; the AP of a class the data set lacks is
    NaN.  More than 1024 detections or ground-truth rows in one image raise ValueError before any launch.

    With `params.aos`: `aos` [..., 41] (NaN in the metrics other than 2D), `aos_r40`, `aos_r11`, `sim_sum` [..., 41] (the fixed-point
    orientation sums, units of 2^-40) and `n_unoriented`, the ground-truth rows of the evaluated classes without a heading (no `alpha`
    key and no valid cuboid); `results()` gains the 'AOS|R40-car-moderate' rows and `summarize()` the devkit's `aos` line after `bbox`."""

    def __init__(self, gt, dt, names=None, params=None, img_ids=None):
        self.gt, self.dt, self.names, self.img_ids = gt, dt, names, img_ids
        self.params = params if params is not None else KittiParams()
        self.eval, self.problem = {}, None

    def _detections(self):
        dt = self.dt
        if isinstance(dt, str):
            with open(dt) as f:
                dt = json.load(f)
        if not isinstance(dt, (list, tuple)):
            dt = dt.loadAnns(dt.getAnnIds()) if hasattr(dt, "getAnnIds") else list(dt.anns.values())
        return dt

    def evaluate(self, device=None):
        p = self.params
        p.check()
        img_ids, by_img, name_of, known = _gt_records(self.gt, self.names)
        if self.img_ids is not None:
            keep = set(self.img_ids)
            img_ids = [i for i in img_ids if i in keep]
        classes = [c.lower() for c in p.classes]
        dontcare = {n.lower() for n in p.dontcareNames}
        # class codes: one per name, and one more per class for its rows that are set aside
        code_of = {}

        def code(name, aside=False):
            return code_of.setdefault((name, aside), len(code_of))

        dts_by = {i: [] for i in img_ids}
        for d in self._detections():
            if d["image_id"] in dts_by:
                dts_by[d["image_id"]].append(d)
        rows_d, rows_g, rows_c = [], [], []
        dt_sizes, gt_sizes, dc_sizes = [], [], []
        for i in img_ids:
            ds = dts_by[i]
            order = np.argsort([-float(x["score"]) for x in ds], kind="mergesort")
            ds = [ds[k] for k in order]
            g_rows, c_rows = [], []
            for a in by_img[i]:
                n = name_of(a)
                if n in dontcare:
                    c_rows.append(a)
                else:
                    aside = n in classes and bool(a.get("ignore") or a.get("ignore2D") or a.get("ignore3D"))
                    g_rows.append((a, code(n, aside)))
            rows_d += [(x, code(name_of(x))) for x in ds]
            rows_g += g_rows
            rows_c += c_rows
            dt_sizes.append(len(ds)), gt_sizes.append(len(g_rows)), dc_sizes.append(len(c_rows))
        dt_sizes, gt_sizes, dc_sizes = (np.array(v, dtype=np.int64) for v in (dt_sizes, gt_sizes, dc_sizes))
        for sizes, what in ((dt_sizes, "detections"), (gt_sizes, "ground-truth rows")):
            if sizes.max(initial=0) > K.MAX_ROWS:
                raise ValueError("image %s has %d %s; the KITTI matching kernels hold %d per image"
                                 % (img_ids[int(sizes.argmax())], int(sizes.max()), what, K.MAX_ROWS))
        cls_tab = np.full((len(classes), max(len(code_of), 1)), -1, dtype=np.int32)
        for (n, aside), k in code_of.items():
            for c, cname in enumerate(classes):
                if n == cname:
                    cls_tab[c, k] = 2 if aside else 0
                elif n in {x.lower() for x in p.neighbours.get(p.classes[c], ())}:
                    cls_tab[c, k] = 1
        if device is None:
            device = torch.device("cpu") if iou3d._lib.get().emulated else torch.device("cuda")
        to = lambda v, dt, shape=(-1,): torch.from_numpy(np.asarray(v, dtype=dt).reshape(shape)).to(device)      # noqa: E731

        def box3d(a):
            b = a.get("bbox3D", a.get("bbox3D_cam"))
            ok = b is not None and bool(a.get("valid3D", True)) and np.asarray(b).shape == (8, 3)
            return b if ok else _NAN_BOX

        b2_d, b2_g, b2_c = (to([list(a["bbox"])[:4] for a in rows], np.float32, (-1, 4)) for rows in
                            ([x for x, _ in rows_d], [x for x, _ in rows_g], rows_c))
        b3_d, b3_g = (to([box3d(x) for x, _ in rows], np.float32, (-1, 8, 3)) for rows in (rows_d, rows_g))
        # pair lists per image, the detections running fastest: (ground-truth row, detection), (DontCare region, detection)
        i_g, i_d, off = _ragged_pairs(gt_sizes, dt_sizes)
        pairs = (i_d, i_g, off)
        zeros = lambda dev: torch.zeros(0, dtype=torch.float32, device=dev)      # noqa: E731
        sims = []
        for m in p.metrics:
            if m == "2D":
                launch = lambda dt, gt, idx1, idx2, _: _xywh_iou(b2_d[idx1.long()], b2_g[idx2.long()])      # noqa: E731
            elif m == "BEV":
                launch = lambda dt, gt, idx1, idx2, _: bev.bev_iou_pairs(bev.bev_footprints(dt, p.up), bev.bev_footprints(gt, p.up), idx1, idx2)      # noqa: E731
            else:
                launch = lambda dt, gt, idx1, idx2, _: iou3d.iou_box3d_exact_pairs(dt, gt, idx1, idx2)[1]      # noqa: E731
            sims.append(_pairs_pass(b3_d, b3_g, dt_sizes, gt_sizes, pairs, zeros, launch)[0])
        sim = torch.stack(sims).contiguous() if sims else torch.zeros((0, int(off[-1])), dtype=torch.float32, device=device)
        c_r, c_d, c_off = _ragged_pairs(dc_sizes, dt_sizes)
        if int(c_off[-1]):
            bd, bc = b2_d[torch.from_numpy(c_d).to(device)], b2_c[torch.from_numpy(c_r).to(device)]
            iw = (torch.min(bd[:, 0] + bd[:, 2], bc[:, 0] + bc[:, 2]) - torch.max(bd[:, 0], bc[:, 0])).clamp(min=0)
            ih = (torch.min(bd[:, 1] + bd[:, 3], bc[:, 1] + bc[:, 3]) - torch.max(bd[:, 1], bc[:, 1])).clamp(min=0)
            area = bd[:, 2] * bd[:, 3]
            dc_ov = torch.where(area > 0, iw * ih / area, torch.zeros_like(area)).contiguous()
        else:
            dc_ov = zeros(device)
        trunc = [max(float(a.get("truncation", -1)), 0.0) for a, _ in rows_g]
        osets = list(p.minOverlaps)
        self.problem = pb = K.Problem(
            dt_sizes, gt_sizes, dc_sizes, sim, dc_ov, to([c for _, c in rows_d], np.int32), to([float(x["bbox"][3]) for x, _ in rows_d], np.float64),
            to([float(x["score"]) for x, _ in rows_d], np.float64), to([c for _, c in rows_g], np.int32),
            to([float(a["bbox"][3]) for a, _ in rows_g], np.float64), to([occlusion_level(a, p.occCuts) for a, _ in rows_g], np.int32),
            to(trunc, np.float64), cls_tab, [[float(h), float(o), float(t)] for _, h, o, t in p.difficulties],
            np.array([p.minOverlaps[o] for o in osets], dtype=np.float64).reshape(len(osets), len(classes)), [m in p.dcMetrics for m in p.metrics])
        keys = ("n_gt", "K", "thresholds", "counts", "precision", "recall", "ap")
        if p.aos:
            # a record's own `alpha` wins; the others take theirs from the corners, all cuboids in one launch (NaN without a valid one)
            own_d, own_g = (to([record_alpha(x) for x, _ in rows], np.float64) for rows in (rows_d, rows_g))
            from_box = K.box_params(torch.cat([b3_d, b3_g]).contiguous(), p.up)[:, 7]
            dt_alpha = torch.where(torch.isnan(own_d), from_box[:len(rows_d)], own_d).contiguous()
            gt_alpha = torch.where(torch.isnan(own_g), from_box[len(rows_d):], own_g).contiguous()
            out = K.run_aos(pb, dt_alpha, gt_alpha, [m == "2D" for m in p.metrics], p.nSamplePts)
            out["gt_alpha"] = gt_alpha
            keys += ("sim_sum", "aos", "aos_ap", "gt_alpha")
        else:
            out = K.run(pb, p.nSamplePts)
        shape = (len(classes), len(p.difficulties), len(p.metrics), len(osets))
        host = {k: out[k].cpu().numpy() for k in keys}      # the one synchronisation
        ap = host["ap"].reshape(shape + (2,)).copy()
        self.lacking = [c for c in classes if c not in known]
        for c, cname in enumerate(classes):
            if cname in self.lacking:
                ap[c] = np.nan
        self.eval = {"precision": host["precision"].reshape(shape + (-1,)), "recall": host["recall"].reshape(shape + (-1,)),
                     "thresholds": host["thresholds"].reshape(shape + (-1,)), "counts": host["counts"].reshape(shape + (-1, 3)),
                     "n_gt": host["n_gt"].reshape(shape), "K": host["K"].reshape(shape), "ap_r40": ap[..., 0], "ap_r11": ap[..., 1],
                     "classes": classes, "difficulties": [d[0] for d in p.difficulties], "metrics": list(p.metrics), "overlaps": osets}
        if p.aos:
            aos_ap = host["aos_ap"].reshape(shape + (2,)).copy()
            for c, cname in enumerate(classes):
                if cname in self.lacking:
                    aos_ap[c] = np.nan
            # ground-truth rows of the evaluated classes without a heading: each can only ever contribute 0
            of_class = np.array([n in classes for (n, _), _ in sorted(code_of.items(), key=lambda kv: kv[1])] + [False], dtype=bool)
            codes_g = np.array([c for _, c in rows_g], dtype=np.int64)
            self.eval.update({"aos": host["aos"].reshape(shape + (-1,)), "aos_r40": aos_ap[..., 0], "aos_r11": aos_ap[..., 1],
                              "sim_sum": host["sim_sum"].reshape(shape + (-1,)),
                              "n_unoriented": int((of_class[codes_g] & ~np.isfinite(host["gt_alpha"])).sum())})
        return self.eval

    def results(self, r11=False):
        """-> {'AP3D|R40-car-moderate': value, ...}: every (metric, class, difficulty) of the first overlap set under its plain name, of
        the other sets with '@<set>' appended; with r11 the '|R11' rows too"""
        e, out = self.eval, {}
        for tag, key in (("R40", "ap_r40"),) + ((("R11", "ap_r11"),) if r11 else ()):
            for o, oname in enumerate(e["overlaps"]):
                for m, metric in enumerate(e["metrics"]):
                    for c, cname in enumerate(e["classes"]):
                        for d, dname in enumerate(e["difficulties"]):
                            out["%s|%s-%s-%s%s" % (METRIC_NAMES[metric][1], tag, cname, dname, "" if o == 0 else "@" + oname)] = float(e[key][c, d, m, o])
                if "aos_r40" in e:                  # with `aos`: the orientation rows of the 2D matching
                    m = e["metrics"].index("2D")
                    for c, cname in enumerate(e["classes"]):
                        for d, dname in enumerate(e["difficulties"]):
                            out["AOS|%s-%s-%s%s" % (tag, cname, dname, "" if o == 0 else "@" + oname)] = float(e["aos_" + tag.lower()][c, d, m, o])
        return out

    def summarize(self, r11=False, overlaps=None, verbose=True):
        """prints and returns the devkit-style table: per class and overlap set (`overlaps`: the names to show, default all) one head
        line and the lines `bbox`, `bev`, `3d` with Easy / Moderate / Hard at R40; r11 adds the R11 block"""
        e, p = self.eval, self.params
        if not e:
            raise Exception("Please run evaluate() first")
        lines = []
        for c, cname in enumerate(e["classes"]):
            for o, oname in enumerate(e["overlaps"]):
                if overlaps is not None and oname not in overlaps:
                    continue
                for tag, key in (("R40", "ap_r40"),) + ((("R11", "ap_r11"),) if r11 else ()):
                    mo = p.minOverlaps[oname][c]
                    lines.append("%s AP|%s@%.2f (%s; %s):" % (cname.capitalize(), tag, mo, oname, ", ".join(e["difficulties"])))
                    for m, metric in enumerate(e["metrics"]):
                        lines.append("%-4s AP:%s" % (METRIC_NAMES[metric][0], ", ".join("%.4f" % v for v in e[key][c, :, m, o])))
                        if metric == "2D" and "aos_r40" in e:
                            lines.append("%-4s AP:%s" % ("aos", ", ".join("%.4f" % v for v in e["aos_" + tag.lower()][c, :, m, o])))
        if e.get("n_unoriented"):
            lines.append("AOS: %d ground-truth rows of the evaluated classes have no heading; a true positive on one adds 0" % e["n_unoriented"])
        text = "\n".join(lines)
        if verbose:
            print(text)
        return text
