"""The prediction plumbing around `Omni3Deval`: instances -> COCO-style records, the inference loop, and the per-split drivers
`tools/train_net.py:do_test` uses, `Omni3DEvaluator` and `Omni3DEvaluationHelper`."""
import copy
import json
import logging
import os

import numpy as np
import torch

from .bootstrap_stats import _bootstrap_ci, _bootstrap_params
from .error_types import _error_params, error_summary
from .modes import MODES, _mean, _percent, _table_ap, check_options, enabled_modes
from .omni3d_evaluation import AnnotationIndex, Omni3Deval
from .pairs import BEV_UP


def _kitti_options(eval_kitti, kitti_params, kitti_r11):
    """the checked `eval_kitti` options of the drivers: None when the switch is off, else (dict of `KittiParams` attributes, r11)"""
    if not eval_kitti:
        return None
    from .kitti import KittiParams
    params = dict(kitti_params or {})
    unknown = set(params) - set(vars(KittiParams()))
    if unknown:
        raise ValueError("kitti_params: unknown keys %s" % sorted(unknown))
    return params, bool(kitti_r11)


def _kitti_pass(gt, dt, options, only_2d, names=None, img_ids=None):
    """the KITTI-protocol pass of the drivers (`cubercnn.evaluation.kitti.KittiEval`) -> (rows {'AP3D|R40-car-moderate': ...}, the table's text, the KittiEval)"""
    from .kitti import KittiEval
    params, r11 = options
    ev = KittiEval(gt, dt, names=names, img_ids=img_ids)
    for key, value in params.items():
        setattr(ev.params, key, value)
    if only_2d:
        ev.params.metrics = ("2D",)
    ev.evaluate()
    return ev.results(r11=r11), ev.summarize(r11=r11, verbose=False), ev


def instances_to_coco_json(instances, img_id):
    """omni3d_evaluation.py:970-1013.  The reference converts each field with its own `.tolist()` after a per-field device
    copy and averages the corner depths one box at a time in numpy; here one host copy per field and a vectorised depth."""
    n = len(instances)
    if n == 0:
        return []
    cpu = instances.to("cpu") if instances.pred_boxes.tensor.is_cuda else instances
    xyxy = cpu.pred_boxes.tensor.numpy()
    boxes = np.concatenate([xyxy[:, :2], xyxy[:, 2:] - xyxy[:, :2]], axis=1).tolist()          # XYXY_ABS -> XYWH_ABS
    scores, classes = cpu.scores.tolist(), cpu.pred_classes.tolist()
    if cpu.has("pred_bbox3D"):
        b3 = cpu.pred_bbox3D.numpy()
        depth = b3[:, :, 2].mean(axis=1).tolist()
        bbox3D, center_cam, center_2D = b3.tolist(), cpu.pred_center_cam.tolist(), cpu.pred_center_2D.tolist()
        dimensions, pose = cpu.pred_dimensions.tolist(), cpu.pred_pose.tolist()
    else:
        bbox3D, center_cam, center_2D = np.ones([n, 8, 3]).tolist(), np.ones([n, 3]).tolist(), np.ones([n, 2]).tolist()
        dimensions, pose, depth = np.ones([n, 3]).tolist(), np.ones([n, 3, 3]).tolist(), [1.0] * n
    return [{"image_id": img_id, "category_id": classes[k], "bbox": boxes[k], "score": scores[k], "depth": depth[k], "bbox3D": bbox3D[k],
             "center_cam": center_cam[k], "center_2D": center_2D[k], "dimensions": dimensions[k], "pose": pose[k]} for k in range(n)]


def inference_on_dataset(model, data_loader):
    """omni3d_evaluation.py:522-640 without the timing / logging: model in eval mode over the loader -> list of
    {'image_id', 'K', 'width', 'height', 'instances': [COCO-style records]}"""
    was_training = model.training
    model.eval()
    out = []
    with torch.no_grad():
        for inputs in data_loader:
            outputs = model(inputs)
            for inp, o in zip(inputs, outputs):
                out.append({"image_id": inp["image_id"], "K": inp["K"], "width": inp["width"], "height": inp["height"],
                            "instances": instances_to_coco_json(o["instances"], inp["image_id"])})
    model.train(was_training)
    return out


def _derive_results(ev, mode, class_names):
    """omni3d_evaluation.py:765-846: the seven headline numbers (x100, NaN when undefined) + per-category AP ('AP-<name>': mean
    of the precision table over thresholds and recall points at area 'all', maxDets 100), each followed by the mode's own keys"""
    M = MODES[mode]
    res = {name: _percent(ev.stats[i]) for i, name in enumerate(M.metrics)}
    res.update(M.derive(ev))
    if class_names is None or len(class_names) <= 1:
        return res
    prec = ev.eval["precision"]
    assert len(class_names) == prec.shape[2], (len(class_names), prec.shape)
    for k, name in enumerate(class_names):
        res["AP-" + name] = _table_ap(prec, k)
        res.update(M.derive_category(ev, k, name))
    return res


def _make_eval(gt, dt, mode, eval_prox, opts):
    """the Omni3Deval of one pass of the drivers, `opts` from `check_options`: `up` is the BEV ground plane, except in mode DIST,
    which has its own"""
    ev = Omni3Deval(gt, dt, mode=mode, eval_prox=eval_prox, up=opts[MODES[mode].up_option])
    MODES[mode].set_pass_params(ev.params, opts)
    return ev


def _agnostic_pass(ev):
    """the class-agnostic pass of a mode (`params.useCats = 0`) on a freshly made evaluator -> (the mode's seven headline APs under
    their usual names and AR1 / AR10 / AR100, all x100 and NaN when undefined; the summary text)"""
    ev.params.useCats = 0
    ev.evaluate()
    ev.accumulate()
    text = ev.summarize()
    res = {name: _percent(ev.stats[i]) for i, name in enumerate(ev._mode.metrics)}
    res.update({"AR%d" % m: _percent(ev.stats[7 + i]) for i, m in enumerate((1, 10, 100))})
    return res, text


class Omni3DEvaluator:
    """Per-dataset evaluator (reference :643-935, a detectron2 COCOEvaluator subclass).

    Reference form: `Omni3DEvaluator(dataset_name, output_dir=..., filter_settings=..., only_2d=..., eval_prox=..., distributed=...)`
    -- the ground truth is the dataset's registered annotation file read through `Omni3D([json_file], filter_settings)`;
    predictions are per-image dicts {'image_id', 'K', 'width', 'height', 'instances': [records with CONTIGUOUS category ids]}.
    `evaluate()` maps the categories back to dataset ids, keeps the dataset's own categories, writes
    `omni_instances_results.json`, runs Omni3Deval in 2D (and 3D) and returns {'bbox_2D': {...}, 'bbox_3D': {...},
    'log_str_2D', 'log_str_3D', 'bbox_*_merge'} ('*_merge' = what the helper needs to score the union of several datasets; the
    reference caches per-image match tables under '*_evals_per_cat_area' for the same purpose).

    Short form (in-memory ground truth): `Omni3DEvaluator(gt_annotations, img_ids, cat_ids, only_2d)` with
    `process(inputs, outputs)` taking model outputs -> {'bbox': {'AP2D', 'AP3D', 'omni_eval_*'}}.

    eval_bev (extension, off by default; `bev_up` = the up vector of the ground plane in the camera frame): unless only_2d, a third
    pass in mode 'BEV' adds 'bbox_BEV', 'log_str_BEV', 'bbox_BEV_merge' (short form: 'APBEV', 'omni_eval_BEV'); nothing else changes.

    eval_dist (extension, off by default; `dist_up` = None for the full 3D distance or the up vector of the ground plane; `dist_params`
    = optional dict of `distThrs` / `tpDist` / `minRecall` set on the pass's params): unless only_2d, one more pass in mode 'DIST'
    after 3D and BEV adds 'bbox_DIST' (the headline APs, 'AP-<name>', 'ATE-<name>', 'ASE-<name>', 'AOE-<name>', 'mATE', 'mASE',
    'mAOE'), 'log_str_DIST', 'bbox_DIST_merge' (short form: 'APDIST', 'omni_eval_DIST'); nothing else changes.

    eval_let (extension, off by default; `let_params` = optional dict of `lonTolFrac` / `lonTolMin` set on the pass's params): unless
    only_2d, one more pass in mode 'LET' after 3D, BEV and DIST adds 'bbox_LET' (LET-AP in the headline slots of the 3D protocol,
    LET-APL as 'APL', 'APL15', ..., 'AP-<name>', 'APL-<name>', 'mAFF', 'mLON'), 'log_str_LET', 'bbox_LET_merge' (short form: 'APLET',
    'omni_eval_LET'); nothing else changes.

    bootstrap (extension, off by default; None or a dict with some of `n` (1000), `seed` (0), `confidence` (0.95)): every evaluated
    mode also gets 'bbox_<mode>_ci': the image-level bootstrap percentile intervals (`Omni3Deval.bootstrap`) of the seven headline
    numbers of 'bbox_<mode>' and of 'AP-<name>' per category, each (lo, hi) x 100 (short form: 'AP<mode>_ci'); nothing else changes.

    errors (extension, off by default; None or a dict with some of `t_fg`, `t_bg`, applied to the modes of the 3D protocol -- mode 2D
    keeps its own): every evaluated mode except DIST also gets 'bbox_<mode>_errors' = the error decomposition of
    `Omni3Deval.errors`: {'t_fg', 't_bg', 'counts': {type: n}, 'dAP': {oracle: mean dAP x 100}, 'loc_errors': {'trans', 'scale',
    'orient'} or None in 2D} (short form: 'errors_<mode>'); nothing else changes.

    eval_agnostic (the reference evaluator's `useCats = 0`, off by default): every evaluated mode gets a second pass with
    `params.useCats = 0` after its ordinary one -- one group per image, the categories ignored -- which adds 'bbox_<mode>_agnostic' =
    the mode's seven headline APs under their usual names plus 'AR1', 'AR10', 'AR100', and 'log_str_<mode>_agnostic' (short form:
    'agnostic_<mode>'); nothing else changes.

    eval_kitti (extension, off by default; `kitti_params` = optional dict of `KittiParams` attributes such as `occCuts` / `dcMetrics`,
    `kitti_r11` adds the 11-point rows): after the modes, one pass of the KITTI object benchmark's own protocol
    (`cubercnn.evaluation.kitti.KittiEval`; with only_2d its 2D metric alone) adds 'bbox_KITTI' = {'AP3D|R40-car-moderate': ..., ...} and
    'log_str_KITTI' = the devkit-style table (short form: 'KITTI' and 'kitti_eval' under 'bbox'; the short form's records need
    `category_name`, or `kitti_names` = category id -> name); nothing else changes."""

    def __init__(self, dataset_name, tasks=None, distributed=True, output_dir=None, *, max_dets_per_image=None, use_fast_impl=False,
                 eval_prox=False, only_2d=False, filter_settings=None, img_ids=None, cat_ids=None, eval_bev=False, bev_up=BEV_UP,
                 eval_dist=False, dist_up=None, dist_params=None, eval_let=False, let_params=None, bootstrap=None, errors=None,
                 eval_agnostic=False, eval_kitti=False, kitti_params=None, kitti_r11=False, kitti_names=None):
        self._only_2d, self._eval_prox, self._output_dir, self._distributed = only_2d, eval_prox, output_dir, distributed
        self._eval_agnostic = bool(eval_agnostic)
        self._kitti, self._kitti_names = _kitti_options(eval_kitti, kitti_params, kitti_r11), kitti_names
        self._bootstrap, self._errors = _bootstrap_params(bootstrap), _error_params(errors)
        self._opts = check_options(let_params=let_params, bev_up=bev_up, dist_up=dist_up, dist_params=dist_params)
        self._switches = {"eval_bev": bool(eval_bev), "eval_dist": bool(eval_dist), "eval_let": bool(eval_let)}
        if not isinstance(dataset_name, str):                   # short form: (gt_annotations, img_ids, cat_ids, only_2d)
            self._gt, self._omni_api = dataset_name, None
            self._img_ids = tasks if tasks is not None else img_ids
            self._cat_ids = cat_ids if isinstance(distributed, bool) else distributed
            if output_dir is not None and not isinstance(output_dir, str):
                self._only_2d, self._output_dir = bool(output_dir), None
            self.reset()
            return
        from ...d2.data import MetadataCatalog
        from ..data.datasets import Omni3D
        self._filter_settings = filter_settings if filter_settings is not None else {}
        self._metadata = MetadataCatalog.get(dataset_name)
        self._omni_api = Omni3D([self._metadata.json_file], self._filter_settings)
        self._do_evaluation = "annotations" in self._omni_api.dataset
        self.reset()

    def reset(self):
        self._predictions = []
        self._results = {}

    def process(self, inputs, outputs):
        for inp, o in zip(inputs, outputs):
            recs = o["instances"] if isinstance(o["instances"], list) else instances_to_coco_json(o["instances"], inp["image_id"])
            if self._omni_api is None:
                self._predictions.extend(recs)
            else:
                pred = {"image_id": inp["image_id"], "K": inp["K"], "width": inp["width"], "height": inp["height"], "instances": recs}
                if "p2" in inp:
                    pred["p2"] = inp["p2"]
                self._predictions.append(pred)

    def _modes(self):
        return enabled_modes(self._only_2d, **self._switches)

    def _make_eval(self, gt, dt, mode, eval_prox=False):
        return _make_eval(gt, dt, mode, eval_prox, self._opts)

    def _evaluate_short(self):
        res = {}
        for mode in self._modes():
            ev = self._make_eval(AnnotationIndex(copy.deepcopy(self._gt), self._img_ids, self._cat_ids),
                                 AnnotationIndex(copy.deepcopy(self._predictions), self._img_ids, self._cat_ids), mode)
            ev.evaluate()
            ev.accumulate()
            ev.summarize()
            res["AP" + mode] = float(ev.stats[0] * 100)
            res["omni_eval_" + mode] = ev
            if self._bootstrap is not None:
                res["AP" + mode + "_ci"] = _bootstrap_ci(ev, mode, None, self._bootstrap)["AP"]
            if self._errors is not None and MODES[mode].error_thrs is not None:
                res["errors_" + mode] = error_summary(ev, self._errors)
            if self._eval_agnostic:
                res["agnostic_" + mode] = _agnostic_pass(self._make_eval(AnnotationIndex(copy.deepcopy(self._gt), self._img_ids, self._cat_ids),
                                                                         AnnotationIndex(copy.deepcopy(self._predictions), self._img_ids, self._cat_ids), mode))[0]
        if self._kitti is not None:
            res["KITTI"], _, res["kitti_eval"] = _kitti_pass(AnnotationIndex(copy.deepcopy(self._gt), self._img_ids, self._cat_ids),
                                                             copy.deepcopy(self._predictions), self._kitti, self._only_2d, self._kitti_names)
        return {"bbox": res}

    def evaluate(self, img_ids=None):
        if self._omni_api is None:
            return self._evaluate_short()
        from ...d2.data import MetadataCatalog
        predictions = self._predictions
        if self._distributed:
            from ...d2 import comm
            comm.synchronize()
            gathered = comm.gather(predictions, dst=0)
            predictions = [x for part in gathered for x in part]
            if not comm.is_main_process():
                return {}
        self._results = {}
        if len(predictions) == 0:
            logging.getLogger(__name__).warning("[Omni3DEvaluator] Did not receive valid predictions.")
            return {}
        if self._output_dir:
            os.makedirs(self._output_dir, exist_ok=True)
            torch.save(predictions, os.path.join(self._output_dir, "instances_predictions.pth"))
        model_meta = MetadataCatalog.get("omni3d_model")
        model_classes = model_meta.thing_classes
        # the split's own tables are filled in when its dataset dicts are loaded (load_omni3d_json); without a loader run the
        # model's id table and the categories of the annotation file stand in (they are what the loader would have stored)
        id_map = self._metadata.get("thing_dataset_id_to_contiguous_id") or model_meta.thing_dataset_id_to_contiguous_id
        split_classes = self._metadata.get("thing_classes") or [c["name"] for c in sorted(self._omni_api.dataset["categories"], key=lambda c: c["id"])]
        to_dataset_id = {v: k for k, v in id_map.items()}
        num_classes = len(to_dataset_id)
        kept = []
        for rec in (r for pred in predictions for r in pred["instances"]):
            c = rec["category_id"]
            assert c < num_classes, f"A prediction has class={c}, but the model only has {num_classes} classes"
            if model_classes[c] in split_classes:                         # categories this dataset is annotated for
                r = dict(rec)
                r["category_id"] = to_dataset_id[c]
                kept.append(r)
        if self._output_dir:
            with open(os.path.join(self._output_dir, "omni_instances_results.json"), "w") as f:
                json.dump(kept, f)
        if not self._do_evaluation or len(kept) == 0:
            return copy.deepcopy(self._results)
        omni_dt = self._omni_api.loadRes(kept)
        for mode in self._modes():
            ev = self._make_eval(self._omni_api, omni_dt, mode, self._eval_prox)
            if img_ids is not None:
                ev.params.imgIds = img_ids
            ev.evaluate()
            ev.accumulate()
            self._results["log_str_" + mode] = ev.summarize()
            self._results["bbox_" + mode] = _derive_results(ev, mode, split_classes)
            if self._bootstrap is not None:
                self._results["bbox_" + mode + "_ci"] = _bootstrap_ci(ev, mode, split_classes, self._bootstrap)
            if self._errors is not None and MODES[mode].error_thrs is not None:
                self._results["bbox_" + mode + "_errors"] = error_summary(ev, self._errors)
            self._results["bbox_" + mode + "_merge"] = {"gt": self._omni_api, "dt": kept, "eval_prox": self._eval_prox,
                                                        "img_ids": list(ev.params.imgIds), "cat_ids": list(ev.params.catIds)}
            if self._eval_agnostic:
                ev = self._make_eval(self._omni_api, omni_dt, mode, self._eval_prox)
                if img_ids is not None:
                    ev.params.imgIds = img_ids
                self._results["bbox_" + mode + "_agnostic"], self._results["log_str_" + mode + "_agnostic"] = _agnostic_pass(ev)
        if self._kitti is not None:
            self._results["bbox_KITTI"], self._results["log_str_KITTI"], _ = _kitti_pass(self._omni_api, copy.deepcopy(kept), self._kitti,
                                                                                         self._only_2d, self._kitti_names, img_ids)
        return copy.deepcopy({k: v for k, v in self._results.items() if not k.endswith("_merge")}) | \
            {k: v for k, v in self._results.items() if k.endswith("_merge")}


class Omni3DEvaluationHelper:
    """omni3d_evaluation.py:168-520: one `Omni3DEvaluator` per test split, their printed tables, and `summarize_all()` = the
    metrics of the union of all splits (<Concat>) plus the Omni3D / Omni3D_In / Omni3D_Out aggregates.  Needs
    `MetadataCatalog.get('omni3d_model').{thing_classes, thing_dataset_id_to_contiguous_id}`.  The union is scored by one
    evaluation over the concatenated ground truth and detections (images of different splits are disjoint, so this equals the
    reference's concatenation of cached per-image match tables), with proximity evaluation applied to the images of the splits
    that use it.

    bootstrap (extension, off by default; None or the dict `Omni3DEvaluator` takes): every split's result gets 'bbox_<mode>_ci', and
    `results_ci[name]` = {'iters', 'AP2D': (lo, hi), 'AP3D': (lo, hi)}: the bootstrap intervals (x 100) of the evaluator's AP in modes
    2D and 3D, i.e. of the mean of the per-category APs the AP2D / AP3D columns show.  For <Concat> the images are resampled within
    the split they come from (strata), so every replicate keeps the splits' sizes.  The printed tables do not change.

    errors (extension, off by default; None or the dict `Omni3DEvaluator` takes): every split's result gets 'bbox_<mode>_errors' for
    every evaluated mode except DIST, `results_errors[name]` = {'iters', '<mode>': {oracle: mean dAP x 100}, ...}, and one log line
    per split.  The printed tables do not change.

    eval_agnostic (off by default; the switch `Omni3DEvaluator` takes): every split's result gets 'bbox_<mode>_agnostic' and
    'log_str_<mode>_agnostic', `results_agnostic[name]` = {'iters', '<mode>': {the seven headline APs, 'AR1', 'AR10', 'AR100'}, ...}
    per split and for <Concat>, and one log line per split.  The printed tables do not change.

    eval_kitti (off by default; `kitti_params`, `kitti_r11` as `Omni3DEvaluator` takes them): every split's result gets 'bbox_KITTI' and
    'log_str_KITTI', `results_kitti[name]` = {'iters', 'AP3D|R40-car-moderate': ..., ...} per split, and the table is logged.  There is
    no <Concat> row: the protocol belongs to one benchmark's split.  The printed tables do not change."""

    def __init__(self, dataset_names, filter_settings, output_folder, iter_label="-", only_2d=False, eval_bev=False, bev_up=BEV_UP,
                 eval_dist=False, dist_up=None, dist_params=None, eval_let=False, let_params=None, bootstrap=None, errors=None,
                 eval_agnostic=False, eval_kitti=False, kitti_params=None, kitti_r11=False):
        from collections import OrderedDict
        from ...d2.data import MetadataCatalog
        from ..data.datasets import simple_register
        self.dataset_names, self.filter_settings, self.output_folder = list(dataset_names), filter_settings, output_folder
        self.iter_label, self.only_2d = iter_label, only_2d
        self.evaluators, self.results = OrderedDict(), OrderedDict()
        self.results_analysis, self.results_omni3d = OrderedDict(), OrderedDict()
        # extensions (off by default), per split and for <Concat>: AP in the bird's-eye view in `results_bev`; centre-distance AP and
        # ATE / ASE / AOE in `results_dist`; LET-AP / LET-APL and the longitudinal diagnostics in `results_let`
        self.eval_bev, self.eval_dist, self.eval_let = (bool(v) and not only_2d for v in (eval_bev, eval_dist, eval_let))
        self.modes = enabled_modes(only_2d, eval_bev=self.eval_bev, eval_dist=self.eval_dist, eval_let=self.eval_let)
        self._opts = check_options(bev_up=bev_up, dist_up=dist_up, dist_params=dist_params, let_params=let_params)
        for key, value in self._opts.items():                   # public: bev_up, dist_up, dist_params, let_params as checked
            setattr(self, key, value)
        self.results_bev, self.results_dist, self.results_let = OrderedDict(), OrderedDict(), OrderedDict()
        # extension (off by default): bootstrap intervals of AP2D / AP3D per split and for <Concat>, in `results_ci`
        self.bootstrap, self.results_ci = _bootstrap_params(bootstrap), OrderedDict()
        # extension (off by default): the error decomposition of every mode but DIST per split, in `results_errors`
        self.errors, self.results_errors = _error_params(errors), OrderedDict()
        # the reference evaluator's useCats = 0 (off by default): class-agnostic AP / AR of every mode per split and for <Concat>
        self.eval_agnostic, self.results_agnostic = bool(eval_agnostic), OrderedDict()
        # extension (off by default): the KITTI object benchmark's own protocol per split, in `results_kitti`
        self.eval_kitti, self.kitti_params, self.kitti_r11, self.results_kitti = bool(eval_kitti), kitti_params, bool(kitti_r11), OrderedDict()
        _kitti_options(eval_kitti, kitti_params, kitti_r11)
        self.overall_imgIds, self.overall_catIds = set(), set()
        self.output_folders = {n: os.path.join(output_folder, n) for n in self.dataset_names}
        for name in self.dataset_names:
            if MetadataCatalog.get(name).get("json_file") is None:
                simple_register(name, filter_settings, filter_empty=False)
            ev = Omni3DEvaluator(name, output_dir=self.output_folders[name], filter_settings=filter_settings, only_2d=only_2d,
                                 eval_prox=("Objectron" in name or "SUNRGBD" in name), distributed=False, eval_bev=self.eval_bev,
                                 eval_dist=self.eval_dist, eval_let=self.eval_let, bootstrap=self.bootstrap, errors=self.errors,
                                 **({"eval_agnostic": True} if self.eval_agnostic else {}),
                                 **({"eval_kitti": True, "kitti_params": kitti_params, "kitti_r11": kitti_r11} if self.eval_kitti else {}), **self._opts)
            ev.reset()
            self.evaluators[name] = ev
            self.overall_imgIds.update(ev._omni_api.getImgIds())
            self.overall_catIds.update(ev._omni_api.getCatIds())

    def add_predictions(self, dataset_name, predictions):
        self.evaluators[dataset_name]._predictions += predictions

    def save_predictions(self, dataset_name):
        os.makedirs(self.output_folders[dataset_name], exist_ok=True)
        torch.save(self.evaluators[dataset_name]._predictions, os.path.join(self.output_folders[dataset_name], "instances_predictions.pth"))

    def _ci_row(self, c2, c3):
        """the row of `results_ci`: the intervals of the evaluator's AP in modes 2D and 3D"""
        nan2 = (float("nan"), float("nan"))
        return {"iters": self.iter_label, "AP2D": c2["AP"] if c2 else nan2, "AP3D": c3["AP"] if c3 and not self.only_2d else nan2}

    def _analysis_row(self, r2, r3, categories):
        """the row of `results_analysis`: AP2D / AP3D = means of the per-category APs, then the headline columns of mode 3D"""
        nan = float("nan")
        return {"iters": self.iter_label, **self._aggregates(r2, r3, categories),
                **{"AP3D" + col: (r3[k] if not self.only_2d else nan)
                   for col, k in (("@15", "AP15"), ("@25", "AP25"), ("@50", "AP50"), ("-N", "APn"), ("-M", "APm"), ("-F", "APf"))}}

    def _mode_rows(self, label, results, categories):
        """the rows of `results_bev` / `results_dist` / `results_let` from `results(mode)` = the mode's derived dict or None"""
        for mode in self.modes:
            M, r = MODES[mode], results(mode)
            if M.results is not None and r is not None:
                getattr(self, M.results)[label] = M.row(self.iter_label, r, categories)

    def _aggregates(self, res2d, res3d, categories):
        return {"AP2D": _mean(res2d["AP-" + c] for c in categories),
                "AP3D": float("nan") if self.only_2d else _mean(res3d["AP-" + c] for c in categories)}

    def evaluate(self, dataset_name):
        from ..data.datasets import get_omni3d_categories
        from ..vis import logperf
        log = logging.getLogger(__name__)
        if dataset_name not in self.results:
            self.results[dataset_name] = self.evaluators[dataset_name].evaluate()
        res = self.results[dataset_name]
        tag = "{} iter={} mode=".format(dataset_name, self.iter_label)
        for mode in self.modes:                                # an extension's text may be missing, that of 2D and 3D must be there
            if not MODES[mode].extension or "log_str_" + mode in res:
                log.info("\n" + res["log_str_" + mode].replace("mode=" + mode, tag + mode))
        names = self.filter_settings["category_names"]
        r2, r3 = res["bbox_2D"], res.get("bbox_3D", {})
        present = {c for c in names if "AP-" + c in r2}
        general = self._analysis_row(r2, r3, present)
        omni = {"AP2D": float("nan"), "AP3D": float("nan")}
        split_cats = get_omni3d_categories(dataset_name)
        if len(split_cats - present) == 0:
            omni = self._aggregates(r2, r3, split_cats)
        self.results_omni3d[dataset_name] = {"iters": self.iter_label, **omni}
        self.results_analysis[dataset_name] = general
        self._mode_rows(dataset_name, lambda mode: res.get("bbox_" + mode), present)
        if self.bootstrap is not None and "bbox_2D_ci" in res:
            self.results_ci[dataset_name] = self._ci_row(res["bbox_2D_ci"], res.get("bbox_3D_ci"))
            log.info("{} iter={} bootstrap {:g} % intervals (n={}): {}".format(dataset_name, self.iter_label, 100 * self.bootstrap["confidence"],
                                                                            self.bootstrap["n"], self.results_ci[dataset_name]))
        if self.errors is not None and "bbox_2D_errors" in res:
            self.results_errors[dataset_name] = {"iters": self.iter_label, **{mode: res["bbox_" + mode + "_errors"]["dAP"] for mode in self.modes
                                                                               if "bbox_" + mode + "_errors" in res}}
            log.info("{} iter={} error decomposition, dAP per oracle: {}".format(dataset_name, self.iter_label, {
                mode: {k: round(v, 2) for k, v in row.items()} for mode, row in self.results_errors[dataset_name].items() if mode != "iters"}))
        if self.eval_agnostic and "bbox_2D_agnostic" in res:
            self.results_agnostic[dataset_name] = {"iters": self.iter_label, **{mode: res["bbox_" + mode + "_agnostic"] for mode in self.modes
                                                                                 if "bbox_" + mode + "_agnostic" in res}}
            log.info("{} iter={} class-agnostic AP / AR100: {}".format(dataset_name, self.iter_label, {
                mode: (round(row["AP"], 2), round(row["AR100"], 2)) for mode, row in self.results_agnostic[dataset_name].items() if mode != "iters"}))
        if self.eval_kitti and "bbox_KITTI" in res:
            self.results_kitti[dataset_name] = {"iters": self.iter_label, **res["bbox_KITTI"]}
            log.info("{} iter={} KITTI protocol\n{}".format(dataset_name, self.iter_label, res["log_str_KITTI"]))
        logperf.print_ap_category_histogram(dataset_name, self._per_category(r2, r3))

    def _per_category(self, r2, r3):
        from collections import OrderedDict
        out = OrderedDict()
        for c in self.filter_settings["category_names"]:
            a2 = r2.get("AP-" + c, float("nan"))
            a3 = r3.get("AP-" + c, float("nan")) if not self.only_2d else float("nan")
            if not np.isnan(a2) or not np.isnan(a3):
                out[c] = {"AP2D": a2, "AP3D": a3}
        return out

    def summarize_all(self):
        from ...d2.data import MetadataCatalog
        from ..data.datasets import get_omni3d_categories
        from ..vis import logperf
        for name in self.dataset_names:
            if name not in self.results:
                self.evaluate(name)
        meta = MetadataCatalog.get("omni3d_model")
        cat_ids = sorted(self.overall_catIds)
        ordered = [meta.thing_classes[meta.thing_dataset_id_to_contiguous_id[c]] for c in cat_ids]
        categories = set(ordered)
        merged, merged_ci, merged_agnostic = {}, {}, {}
        for mode in self.modes:
            gts, dts, prox_imgs, strata = [], [], set(), {}
            for name in self.dataset_names:
                rec = self.results[name].get("bbox_" + mode + "_merge")
                if rec is None:
                    continue
                gts += rec["gt"].loadAnns(rec["gt"].getAnnIds(imgIds=rec["img_ids"], catIds=rec["cat_ids"]))
                dts += rec["dt"]
                if rec["eval_prox"]:
                    prox_imgs.update(rec["img_ids"])
                strata.update({i: name for i in rec["img_ids"]})
            ev = _make_eval(AnnotationIndex(copy.deepcopy(gts), self.overall_imgIds, cat_ids),
                            AnnotationIndex(copy.deepcopy(dts), self.overall_imgIds, cat_ids), mode, (prox_imgs if prox_imgs else False), self._opts)
            ev.evaluate()
            ev.accumulate()
            ev.summarize()
            merged[mode] = _derive_results(ev, mode, ordered if len(ordered) > 1 else None)
            if self.bootstrap is not None and MODES[mode].concat_ci:
                # an image no split lists (it has no prediction record) is a stratum of its own kind
                merged_ci[mode] = _bootstrap_ci(ev, mode, None, self.bootstrap, strata={i: strata.get(i, "") for i in ev.params.imgIds})
            if len(ordered) == 1:
                MODES[mode].single_class(merged[mode], ordered[0])
            if self.eval_agnostic:
                merged_agnostic[mode] = _agnostic_pass(_make_eval(
                    AnnotationIndex(copy.deepcopy(gts), self.overall_imgIds, cat_ids), AnnotationIndex(copy.deepcopy(dts), self.overall_imgIds, cat_ids),
                    mode, (prox_imgs if prox_imgs else False), self._opts))[0]
        r2, r3 = merged["2D"], merged.get("3D", {})
        self._mode_rows("<Concat>", merged.get, categories)
        if "2D" in merged_ci:
            self.results_ci["<Concat>"] = self._ci_row(merged_ci["2D"], merged_ci.get("3D"))
        if self.eval_agnostic:
            self.results_agnostic["<Concat>"] = {"iters": self.iter_label, **merged_agnostic}
        self.results_analysis["<Concat>"] = self._analysis_row(r2, r3, categories)
        for label, key in (("Omni3D_Out", "omni3d_out"), ("Omni3D_In", "omni3d_in"), ("Omni3D", "omni3d")):
            want = get_omni3d_categories(key)
            agg = self._aggregates(r2, r3, want) if len(want - categories) == 0 else {"AP2D": float("nan"), "AP3D": float("nan")}
            self.results_omni3d[label] = {"iters": self.iter_label, **agg}
        logperf.print_ap_category_histogram("<Concat>", self._per_category(r2, r3))
        logperf.print_ap_analysis_histogram(self.results_analysis)
        logperf.print_ap_omni_histogram(self.results_omni3d)
        return self.results_analysis, self.results_omni3d
