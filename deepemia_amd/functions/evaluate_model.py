"""``main.py --task evaluate``: COCO box and mask AP of a trained model on the dataset's test split.

What the reference's user guide describes (docs/user-guide.md, "Model Evaluation") with Detectron2's ``COCOEvaluator`` +
``inference_on_dataset`` semantics (the reference's own ``evaluate_model.py`` cannot run as written: it passes ``rcnn`` in
the ``metadata`` slot of ``choose_and_use_model``).  Every test image goes through the whole-image predictor (800 / 1333
resize, score threshold 0.45, at most 100 detections); the ground truth is rasterised, intersected with the detections and
run-length encoded on the GPU (``deepemia_amd.cocoeval``), and COCOeval's matching runs as one native host call.

That is the **predictor** mode (the default).  The **pipeline** mode (``evaluation: {mode: pipeline}`` in the configuration,
global or per dataset, or ``DEEPEMIA_EVAL_MODE=pipeline``) scores what ``--task inference`` ships instead: every test image
goes through ``functions.inference.final_instances`` -- the class loop with its per-class thresholds, the full-image pass
plus the upscaled tiles, the merges, the 0.7 cross-class pass and the spatial constraints, with the R50 + R101 ensemble
where ``--rcnn combo`` is given and the dataset's settings enable it -- and the final masks are scored.  The pipeline has
no regressed box: a detection's box is ``toBbox`` of its mask's run lengths (``cocoeval.rle_to_bbox``).
``evaluation.max_dets`` (default ``[1, 10, 100]``) is COCOeval's ``maxDets``; micrographs with several hundred particles
need its last entry raised.  ``evaluation.score_frame`` (pipeline mode only) says what the scoring reads: ``planes`` (the
default) full-frame planes, with ``mask_frame: full``; ``crops`` the image's final :class:`CropMaskSet` and a ground truth built
as one too, with ``mask_frame: crop`` or ``crop_direct`` -- rooms are scored, no ``[*, H, W/32]`` tensor is allocated.

``evaluation.boundary_ap: true`` (off by default; both modes, both score frames) adds a third task, ``boundary``: COCO AP with
``min(mask IoU, Boundary IoU)`` as the IoU (Cheng et al., CVPR 2021; the definitions are stated in ``include/deepemia_hip.h``).
The bands of the detections and of the rasterised ground truth come from ``demia_mask_boundary_band`` /
``demia_crop_boundary_band`` in the frame being scored; their width is ``evaluation.boundary_dilation_ratio`` (default 0.02) of
the image diagonal, or ``evaluation.boundary_width`` pixels.  With the switch off nothing of it is launched, allocated or copied.

``evaluation.outline_agreement: true`` (off by default; both modes, both score frames) adds a report beside the AP tables: how
far the outline of every matched detection lies from the outline of its annotation, in pixels.  Per image the pairs are matched
on the host from the ``segm`` IoU table (``cocoeval.outline_match``: IoU >= ``evaluation.outline_iou``, default 0.5; not
COCOeval's matcher), ``demia_mask_outline_agreement`` / ``demia_crop_outline_agreement`` measure them in the frame being scored and
return integers (the definitions are stated in ``include/deepemia_hip.h``), and ``cocoeval.outline_values`` makes ASSD, the RMS
surface distance, Hausdorff, HD95 (it saturates at 127 px), the surface Dice at ``evaluation.outline_tolerance`` px (default 2),
the signed equivalent-diameter error and the relative area error of them.  An image with a pair costs one more device-to-host
copy; an image without one, and a run with the switch off, launch, allocate, copy and write nothing for it.  The AP tables, the
result files and the returned dict are the same with the switch on or off.

``--visualize`` (both modes, both score frames) draws one ERROR MAP per test image -- not Detectron2's ``Visualizer`` picture, whose
look is not reproduced: the detections over the ground truth in the frame being scored, painted on the GPU from the packed words the
scorer holds (``demia_mask_error_map`` / ``demia_crop_error_map``; the definitions are stated in ``include/deepemia_hip.h``).  Per
image the masks are paired as for the outline report (``cocoeval.outline_match`` at ``evaluation.visualize_iou``, default 0.5);
pixels both sides hold are filled in one colour, pixels only a detection holds in a second, pixels only an annotation holds in a
third (weight ``evaluation.visualize_alpha`` of 256, default 96), and the outlines of matched, spurious and missed masks and of
crowd regions are drawn on top, ``evaluation.visualize_line`` pixels wide (1 to 4; default ``cocoeval.error_map_line`` of the
image's size).  The pictures go to ``evaluation_images/<image_id>_<stem>_evaluation.png`` with a ``legend.png``, and
``evaluation_images.csv`` has one row per image: the counts of the pairing and the agree / excess / missing / ignored pixels with
the pixel precision, recall and Dice of them.  An image costs one more device-to-host copy (the picture and the counts) and its PNG
encode; with the flag off nothing is launched, allocated, copied or written for it, and the tables, the result files and the
returned dict are the same with the flag on or off.

Outputs in ``output_dir``: ``metrics.csv`` (``metric,value``, one row per task: ``bbox``, ``segm`` and, when asked for, ``boundary``), ``coco_instances_results.json``
(``instances_to_coco_json`` layout, dataset category ids) and ``instances_predictions.pth``; with the outline report,
``outline_agreement.csv`` (one row per matched pair, in image order, then detection order) and ``outline_summary.csv`` (one row per
class and the row ``all``, pooled over the pairs; a class without a pair has empty value fields); with ``--visualize``,
``evaluation_images/`` and ``evaluation_images.csv``.  Not provided: in predictor mode, the ``combo`` model pair.
"""
from __future__ import annotations

import csv
import json
import os
import time
from collections import OrderedDict
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import cocoeval as CE
from ..cropset import CropMaskSet
from ..data.datasets import (MetadataCatalog, get_split_dicts, load_coco_test, load_or_create_split, read_dataset_info,
                             register_datasets, rle_counts_of)
from ..data.models import choose_and_use_model, get_trained_model_paths
from ..maskset import MaskOps, OutlineAgreement
from ..utils.config import get_config
from ..utils.logger_utils import system_logger

SCORE_THRESH = 0.45          # evaluate_model.py:78 (--threshold does not apply)
BATCH = 4                    # same-size test images per forward
MODES = ("predictor", "pipeline")
SCORE_FRAMES = ("planes", "crops")


def _evaluation_key(dataset_name: Optional[str] = None) -> dict:
    """The ``evaluation`` key of the configuration (global, or merged with the dataset's file); ``{}`` when it is absent."""
    try:
        return (get_config(dataset_name=dataset_name) if dataset_name else get_config()).get("evaluation", {}) or {}
    except FileNotFoundError:        # (no configuration at all: the caller's own read reports it)
        return {}


def evaluation_settings(dataset_name: Optional[str] = None) -> Tuple[str, List[int]]:
    """``(mode, max_dets)`` from the ``evaluation`` key of the configuration (global, or in the dataset's file; neither entry is
    required); ``DEEPEMIA_EVAL_MODE`` overrides the mode.  ValueError for an unknown mode or a malformed ``max_dets``."""
    cfg = _evaluation_key(dataset_name)
    mode = str(os.environ.get("DEEPEMIA_EVAL_MODE") or cfg.get("mode", "predictor")).strip().lower()
    if mode not in MODES:
        raise ValueError(f"evaluation mode must be one of {MODES}, got {mode!r}")
    return mode, CE.check_max_dets(cfg.get("max_dets"))


def score_frame_setting(dataset_name: Optional[str] = None, mask_frame: Optional[str] = None) -> str:
    """``evaluation.score_frame`` (global, or in the dataset's file, next to ``mode`` and ``max_dets``): what the pipeline mode's
    scoring reads, ``planes`` (the default) or ``crops``; the predictor mode never asks.  ValueError for an unknown value and,
    when the dataset's ``mask_frame`` is given, for a pair that does not go together: ``crops`` scores the pipeline's
    :class:`CropMaskSet` and needs ``mask_frame: crop`` or ``crop_direct``; ``planes`` scores planes and needs ``mask_frame: full``."""
    cfg = _evaluation_key(dataset_name)
    frame = str(cfg.get("score_frame", "planes")).strip().lower()
    if frame not in SCORE_FRAMES:
        raise ValueError(f"evaluation.score_frame must be 'planes' or 'crops', got {frame!r}")
    if mask_frame is not None:
        if frame == "crops" and mask_frame == "full":
            raise ValueError("evaluation.score_frame: crops needs inference_settings.mask_frame: crop or crop_direct "
                             "(mask_frame: full hands the scoring planes)")
        if frame == "planes" and mask_frame != "full":
            raise ValueError(f"inference_settings.mask_frame: {mask_frame} is not supported by the evaluate task's pipeline mode with "
                             "evaluation.score_frame: planes (that scoring runs on full-frame planes only); use evaluation.score_frame: "
                             "crops, or mask_frame: full, for this dataset")
    return frame


def boundary_setting(dataset_name: Optional[str] = None) -> Optional[Tuple[float, Optional[int]]]:
    """The boundary-AP switch of the ``evaluation`` key (global, or in the dataset's file): None when ``evaluation.boundary_ap`` is
    false or absent (the default: nothing is launched, allocated or copied for it), else ``(ratio, width)`` --
    ``evaluation.boundary_dilation_ratio`` (default 0.02) and ``evaluation.boundary_width`` (None, or the erosion width in pixels,
    which then replaces the ratio); ``cocoeval.boundary_width`` makes an image's ``d`` of them.  ValueError, with the key named,
    for a wrong type or range; all three keys are checked whether or not the switch is on."""
    cfg = _evaluation_key(dataset_name)
    on = cfg.get("boundary_ap", False)
    if not isinstance(on, bool):
        raise ValueError(f"evaluation.boundary_ap must be true or false, got {on!r}")
    ratio = cfg.get("boundary_dilation_ratio", CE.BOUNDARY_RATIO)
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not (0.0 < float(ratio) < 1.0):
        raise ValueError(f"evaluation.boundary_dilation_ratio must be a number between 0 and 1 (exclusive), got {ratio!r}")
    width = cfg.get("boundary_width")
    if width is not None and (isinstance(width, bool) or not isinstance(width, int) or width < 1):
        raise ValueError(f"evaluation.boundary_width must be an integer >= 1, got {width!r}")
    return (float(ratio), width) if on else None


def outline_setting(dataset_name: Optional[str] = None) -> Optional[Tuple[float, int]]:
    """The outline-agreement switch of the ``evaluation`` key (global, or in the dataset's file): None when
    ``evaluation.outline_agreement`` is false or absent (the default: nothing is launched, allocated, copied or written for it),
    else ``(iou, tolerance)`` -- ``evaluation.outline_iou`` (default 0.5, a number in (0, 1]: the mask IoU from which a detection and
    an annotation are a pair) and ``evaluation.outline_tolerance`` (default 2, an integer from 0 to 126: the surface Dice's
    tolerance in pixels).  ValueError, with the key named, for a wrong type or range; all three keys are checked whether or not
    the switch is on."""
    cfg = _evaluation_key(dataset_name)
    on = cfg.get("outline_agreement", False)
    if not isinstance(on, bool):
        raise ValueError(f"evaluation.outline_agreement must be true or false, got {on!r}")
    iou = cfg.get("outline_iou", CE.OUTLINE_IOU)
    if isinstance(iou, bool) or not isinstance(iou, (int, float)) or not (0.0 < float(iou) <= 1.0):
        raise ValueError(f"evaluation.outline_iou must be a number in (0, 1], got {iou!r}")
    tol = cfg.get("outline_tolerance", CE.OUTLINE_TOLERANCE)
    if isinstance(tol, bool) or not isinstance(tol, int) or not (0 <= tol <= 126):
        raise ValueError(f"evaluation.outline_tolerance must be an integer from 0 to 126, got {tol!r}")
    return (float(iou), int(tol)) if on else None


def visualize_setting(dataset_name: Optional[str] = None) -> Tuple[float, int, Optional[int]]:
    """The error maps' settings of the ``evaluation`` key (global, or in the dataset's file), for ``--visualize``: ``(iou, alpha,
    line)`` -- ``evaluation.visualize_iou`` (default 0.5, a number in (0, 1]: the mask IoU from which a detection and an annotation are
    a pair), ``evaluation.visualize_alpha`` (default 96, an integer from 0 to 256: the fill colours' weight of 256) and
    ``evaluation.visualize_line`` (default unset: ``cocoeval.error_map_line`` of each image; or an integer from 1 to 4, the outlines'
    width in pixels).  ValueError, with the key named, for a wrong type or range; all three keys are checked whether or not the flag
    is given."""
    cfg = _evaluation_key(dataset_name)
    iou = cfg.get("visualize_iou", CE.ERROR_MAP_IOU)
    if isinstance(iou, bool) or not isinstance(iou, (int, float)) or not (0.0 < float(iou) <= 1.0):
        raise ValueError(f"evaluation.visualize_iou must be a number in (0, 1], got {iou!r}")
    alpha = cfg.get("visualize_alpha", CE.ERROR_MAP_ALPHA)
    if isinstance(alpha, bool) or not isinstance(alpha, int) or not (0 <= alpha <= 256):
        raise ValueError(f"evaluation.visualize_alpha must be an integer from 0 to 256, got {alpha!r}")
    line = cfg.get("visualize_line")
    if line is not None and (isinstance(line, bool) or not isinstance(line, int) or not (1 <= line <= 4)):
        raise ValueError(f"evaluation.visualize_line must be an integer from 1 to 4, got {line!r}")
    return float(iou), int(alpha), line


def read_image_bgr(path: str) -> np.ndarray:
    """Detectron2's ``read_image(path, "BGR")``: PIL decode, EXIF orientation applied, converted to RGB, channels reversed."""
    from PIL import Image, ImageOps

    with Image.open(path) as im:
        im = ImageOps.exif_transpose(im)
        return np.ascontiguousarray(np.asarray(im.convert("RGB"))[:, :, ::-1])


def _test_records(dataset_name: str, dataset_format: str, dataset_info: dict, split_dir: Path):
    """(records, class names in category-id order, contiguous id -> dataset category id)."""
    if dataset_format == "json":
        img_dir, label_dir, thing_classes = dataset_info[dataset_name]
        split = load_or_create_split(img_dir, dataset_name, split_dir)
        recs = get_split_dicts(img_dir, label_dir, split["test"], thing_classes)
        return recs, list(thing_classes), {i: i for i in range(len(thing_classes))}
    root = Path(get_config()["paths"].get("local_dataset_root", "~")).expanduser()
    recs, names, id_map = load_coco_test(root / "DATASET" / dataset_name)
    return recs, names, {v: k for k, v in id_map.items()}


def _gt_box_xywh(a: dict) -> List[float]:
    """``convert_to_coco_dict``'s box: XYWH, each value ``round(float(x), 3)``."""
    b = [float(v) for v in a["bbox"]]
    if a.get("bbox_mode", "XYXY_ABS") == "XYXY_ABS":
        b = [b[0], b[1], b[2] - b[0], b[3] - b[1]]
    return [round(v, 3) for v in b]


def evaluate_model(dataset_name: str, output_dir: str, visualize: bool = False, dataset_format: str = "json",
                   rcnn: Union[int, str] = 101, mode: str = "predictor", threshold: float = 0.65) -> "OrderedDict[str, Dict[str, float]]":
    """Score the trained ``rcnn_r<rcnn>`` model of ``dataset_name`` on its test split; returns Detectron2's
    ``OrderedDict(bbox={...}, segm={...})`` and writes the three result files to ``output_dir``.  ``mode="pipeline"`` scores
    the final instances of the tiled inference pipeline instead of the bare predictor's: ``rcnn`` may then be ``"combo"``
    (both models, as ``--task inference`` loads them) and ``threshold`` is the predictors' score threshold (``--threshold``)."""
    t_start = time.perf_counter()
    if mode not in MODES:
        raise ValueError(f"evaluation mode must be one of {MODES}, got {mode!r}")
    if mode == "predictor" and str(rcnn) == "combo":
        raise ValueError("the predictor mode scores one model: rcnn must be 50 or 101")
    boundary = boundary_setting(dataset_name)          # (checked before any model is loaded)
    outline = outline_setting(dataset_name)            # (likewise)
    report = CE.OutlineReport(*outline) if outline is not None else None
    visual = visualize_setting(dataset_name)           # (likewise, whether or not the flag is given)
    maps = CE.ErrorMaps(output_dir, *visual) if visualize else None
    config = get_config()
    max_dets = CE.check_max_dets(_evaluation_key(dataset_name).get("max_dets"))
    split_dir = Path(config["paths"]["split_dir"]).expanduser().resolve()
    category_json = Path(config["paths"]["category_json"]).expanduser().resolve()
    dataset_info = read_dataset_info(category_json)
    register_datasets(dataset_info, dataset_name, dataset_format=dataset_format)
    recs, class_names, to_dataset_id = _test_records(dataset_name, dataset_format, dataset_info, split_dir)
    metadata = MetadataCatalog.get(f"{dataset_name}_train")
    if mode == "pipeline":
        tables = _new_tables(boundary)
        per_image, times = _run_pipeline(dataset_name, recs, metadata, str(split_dir), rcnn, threshold, tables, to_dataset_id, boundary, report,
                                         maps)
        return _write_results(recs, per_image, tables, to_dataset_id, class_names, output_dir, max_dets, t_start, times, "pipeline", report,
                              maps)
    predictor, _ = choose_and_use_model(get_trained_model_paths(str(split_dir), rcnn), dataset_name, SCORE_THRESH, metadata, rcnn)
    if predictor is None:
        raise FileNotFoundError(f"no trained rcnn_r{rcnn} model for dataset {dataset_name} under {split_dir}")
    device = predictor.engine.device
    ops = MaskOps(str(device))
    system_logger.info(f"Evaluating {len(recs)} test images of {dataset_name} (R{rcnn}, score threshold {SCORE_THRESH})")

    t_read = t_fwd = t_score = 0.0
    tables = _new_tables(boundary)
    per_image: Dict[int, dict] = {}
    # same-size images share a forward; the results keep the record order
    order = sorted(range(len(recs)), key=lambda i: (recs[i]["height"], recs[i]["width"], i))
    pos = 0
    while pos < len(order):
        t0 = time.perf_counter()
        group = [order[pos]]
        imgs = [read_image_bgr(recs[order[pos]]["file_name"])]
        pos += 1
        while pos < len(order) and len(group) < BATCH:
            nxt = read_image_bgr(recs[order[pos]]["file_name"])
            if nxt.shape != imgs[0].shape:
                break
            group.append(order[pos])
            imgs.append(nxt)
            pos += 1
        t1 = time.perf_counter()
        batch = torch.from_numpy(np.stack(imgs)).to(device)
        outs = predictor.predict_batch(batch)
        torch.cuda.synchronize(device)
        t2 = time.perf_counter()
        for k, (ri, out) in enumerate(zip(group, outs)):
            per_image[ri] = _score_image(ops, recs[ri], out["instances"], tables, to_dataset_id, boundary, report,
                                         maps=maps, image=batch[k] if maps is not None else None)
        t3 = time.perf_counter()
        t_read += t1 - t0
        t_fwd += t2 - t1
        t_score += t3 - t2

    return _write_results(recs, per_image, tables, to_dataset_id, class_names, output_dir, max_dets, t_start, (t_read, t_fwd, t_score),
                          "forwards", report, maps)


def _new_tables(boundary=None) -> Dict[str, CE.EvalTables]:
    """The tasks' tables in the order of the results: ``bbox``, ``segm`` and, with the boundary-AP switch on, ``boundary``."""
    tables = {"bbox": CE.EvalTables(), "segm": CE.EvalTables()}
    if boundary is not None:
        tables["boundary"] = CE.EvalTables()
    return tables


def _write_results(recs, per_image, tables, to_dataset_id, class_names, output_dir, max_dets, t_start, times, work: str,
                   report: Optional[CE.OutlineReport] = None, maps: Optional[CE.ErrorMaps] = None):
    """COCOeval over the tables of all images, the three result files and the timing line (``work`` names what ``times[1]``
    measured: the predictor's forwards, or the whole inference pipeline of an image).  ``report``: the run's outline-agreement
    report, when asked for -- its two files are written beside the three and its ``all`` row is logged.  ``maps``: the run's error
    maps, when asked for -- their table and legend are written."""
    t_read, t_fwd, t_score = times
    t0 = time.perf_counter()
    predictions = [{"image_id": recs[i]["image_id"], "instances": per_image[i]["instances"]} for i in range(len(recs))]
    coco_results = [dict(r, category_id=to_dataset_id[r["category_id"]]) for p in predictions for r in p["instances"]]
    os.makedirs(output_dir, exist_ok=True)
    torch.save(predictions, os.path.join(output_dir, "instances_predictions.pth"))
    with open(os.path.join(output_dir, "coco_instances_results.json"), "w") as f:
        f.write(json.dumps(coco_results))
        f.flush()
    cat_ids = sorted(to_dataset_id.values())
    results = OrderedDict()
    if not coco_results:
        system_logger.warning("No predictions from the model!")
        for task in tables:
            results[task] = {m: float("nan") for m in CE.METRICS}
    else:
        ev = CE.evaluate(tables, [r["image_id"] for r in recs], cat_ids, max_dets)
        for task in tables:
            system_logger.info(f"Evaluation results for {task}:\n" + "\n".join(CE.summary_lines(ev[task]["stats"], max_dets)))
            results[task] = CE.derive_results(ev[task]["stats"], ev[task]["precision"], class_names)
    t_score += time.perf_counter() - t0
    system_logger.info(f"Evaluation metrics: {results}")
    csv_path = Path(output_dir) / "metrics.csv"
    with open(csv_path, mode="w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["metric", "value"])
        w.writeheader()
        for key, value in results.items():
            w.writerow({"metric": key, "value": value})
    if report is not None:
        t0 = time.perf_counter()
        summary = report.write(output_dir, [to_dataset_id[i] for i in range(len(class_names))], class_names)
        system_logger.info(f"Outline agreement over {len(report.rows)} matched pairs (IoU >= {report.iou}, NSD at {report.tolerance} px): "
                           + ", ".join(f"{k}={v}" for k, v in zip(CE.OUTLINE_SUMMARY_HEADER, summary[-1])))
        t_score += time.perf_counter() - t0
    if maps is not None:
        t0 = time.perf_counter()
        system_logger.info(f"Error maps of {len(maps.rows)} images (IoU >= {maps.iou}, alpha {maps.alpha}) in {maps.image_dir}; table: {maps.write()}")
        t_score += time.perf_counter() - t0
    n = max(1, len(recs))
    system_logger.info(f"Evaluation wall time {time.perf_counter() - t_start:.2f}s: {work} {t_fwd:.3f}s ({1e3 * t_fwd / n:.1f} ms/image), "
                       f"scoring {t_score:.3f}s ({1e3 * t_score / n:.1f} ms/image), image reads {t_read:.3f}s; "
                       f"metrics saved to {csv_path}")
    return results


# ---- the frame being scored -----------------------------------------------------------------------------------------------------
class _ScoreFrame:
    """One image's detections in the frame they are scored in and, after :meth:`ground_truth`, its annotations in the same frame:
    the device work :func:`_score` asks for, and nothing else.  ``hw`` is the image's ``(H, W)``, ``d_bbox_t`` the detections' tight
    boxes on the device, ``gt_area`` the annotations' pixel counts on the device.  An implementation gives ``_ground_truth``,
    ``cross``, ``bands``, ``rle_launch``, ``rle_again``, ``outline``, ``error_map`` and ``empty`` (the frame of an image without a detection).
    Labels are host arrays; a method enqueues without a wait unless it says otherwise."""

    def __init__(self, ops: MaskOps, H: int, W: int, d_bbox_t: torch.Tensor):
        self.ops, self.hw, self.d_bbox_t = ops, (int(H), int(W)), d_bbox_t

    def ground_truth(self, anns: List[dict]) -> List[torch.Tensor]:
        """Build the ground-truth set in annotation order.  Returns the rasteriser's error word (a 1-element device tensor) for the
        caller to fetch with its own tables, or nothing where the word was waited for and checked here."""
        if any(a.get("segmentation") is None for a in anns):
            raise ValueError("ground truth without a segmentation cannot be scored for masks")
        return self._ground_truth(anns, [i for i, a in enumerate(anns) if isinstance(a.get("segmentation"), list)],
                                  [i for i, a in enumerate(anns) if isinstance(a.get("segmentation"), dict)])


class _PlaneFrame(_ScoreFrame):
    """``score_frame: planes`` and the predictor mode: the detections are full-frame planes ``[n, H, W/32]`` and every annotation is
    rasterised into one."""

    def __init__(self, ops: MaskOps, H: int, W: int, packed: torch.Tensor, d_bbox_t: torch.Tensor):
        super().__init__(ops, H, W, d_bbox_t)
        self.packed = packed

    @classmethod
    def empty(cls, ops: MaskOps, H: int, W: int) -> "_PlaneFrame":
        return cls(ops, H, W, torch.zeros((0, H, (W + 31) // 32), dtype=torch.int32, device=ops.device),
                   torch.zeros((0, 4), dtype=torch.int32, device=ops.device))

    def _ground_truth(self, anns, poly_idx, rle_idx):
        ops, (H, W), err = self.ops, self.hw, []
        polys = [anns[i]["segmentation"] for i in poly_idx]
        if not rle_idx:
            self.g_packed, self.gt_area, self.g_bbox_t = CE.rasterize_polygons(ops, polys, H, W, err_out=err)
            return err
        packed, _, _ = CE.rasterize_polygons(ops, polys, H, W)             # (run-length ground truth: its own waits)
        dense = np.stack([CE.rle_decode(rle_counts_of(anns[i]["segmentation"]), H, W) for i in rle_idx])
        self.g_packed = torch.empty((len(anns), H, (W + 31) // 32), dtype=torch.int32, device=ops.device)
        if poly_idx:
            self.g_packed[torch.tensor(poly_idx, device=ops.device)] = packed
        self.g_packed[torch.tensor(rle_idx, device=ops.device)] = ops.from_dense(dense)
        self.gt_area, self.g_bbox_t = ops.area_bbox(self.g_packed)
        return err

    def cross(self, det_labels, gt_labels, det=None, gt=None) -> torch.Tensor:
        """``[n, G]`` intersections of the detections and the annotations (or of the planes ``det`` / ``gt`` in their boxes)."""
        return CE.cross_matrix(self.ops, self.packed if det is None else det, self.d_bbox_t, det_labels,
                               self.g_packed if gt is None else gt, self.g_bbox_t, gt_labels, self.hw[1])

    def bands(self, d: int, det_labels, gt_labels) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The boundary task at width ``d``: (band intersections ``[n, G]``, detection band areas ``[n]``, ground-truth band areas ``[G]``)."""
        d_band, d_ba = self.ops.boundary_band(self.packed, self.d_bbox_t, d, self.hw[1])
        g_band, g_ba = self.ops.boundary_band(self.g_packed, self.g_bbox_t, d, self.hw[1])
        return self.cross(det_labels, gt_labels, d_band, g_band), d_ba, g_ba

    def rle_launch(self, room: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return CE.rle_counts_launch(self.ops, self.packed, self.d_bbox_t, self.hw[1], room)

    def rle_again(self) -> Tuple[np.ndarray, np.ndarray]:
        """The two-pass encoder, for a room that was too small: one more wait."""
        return CE.rle_counts(self.ops, self.packed, self.d_bbox_t, self.hw[1])

    def outline(self, pairs, d_px, g_px) -> OutlineAgreement:
        return self.ops.outline_agreement(self.packed, self.d_bbox_t, d_px, self.g_packed, self.g_bbox_t, g_px, pairs, W=self.hw[1])

    def error_map(self, image, d_state, g_state, alpha: int, line: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The error map of the frame on ``image`` (uint8, on the device): ``(picture [H, W, 3], counts [4] int64)`` on the device."""
        return self.ops.error_map(self.packed, self.d_bbox_t, d_state, self.g_packed, self.g_bbox_t, g_state, image, alpha, line, W=self.hw[1])


class _CropFrame(_ScoreFrame):
    """``score_frame: crops``: the same launches over rooms -- the ground truth becomes a :class:`CropMaskSet` too (polygons are
    rasterised into rooms, run-length annotations are packed on the host), the cross matrix and the run lengths read both sets'
    words in place, and the bands of the boundary task are sets over the same rooms.  No ``[*, H, W/32]`` tensor exists here."""

    def __init__(self, ops: MaskOps, cset: CropMaskSet, d_bbox_t: torch.Tensor):
        super().__init__(ops, *cset.hw, d_bbox_t)
        self.cset = cset

    @classmethod
    def empty(cls, ops: MaskOps, H: int, W: int) -> "_CropFrame":
        cset = CropMaskSet.empty(ops, (H, W))
        return cls(ops, cset, cset.bbox)

    def _ground_truth(self, anns, poly_idx, rle_idx):
        ops, (H, W) = self.ops, self.hw
        self.gt, err = CE.rasterize_polygons_crop(ops, [anns[i]["segmentation"] for i in poly_idx], H, W)
        if rle_idx:
            runs = CE.rle_crop_set(ops, [rle_counts_of(anns[i]["segmentation"]) for i in rle_idx], H, W)
            if poly_idx:
                place = np.empty(len(anns), dtype=np.int64)
                place[poly_idx + rle_idx] = np.arange(len(anns))
                runs = CropMaskSet.cat([self.gt, runs]).select(place)
            self.gt = runs
        self.gt_area = self.gt.area
        return [err]

    def cross(self, det_labels, gt_labels, det=None, gt=None) -> torch.Tensor:
        return CE.cross_matrix_crop(self.ops, self.cset if det is None else det, det_labels, self.gt if gt is None else gt, gt_labels,
                                    det_bbox=self.d_bbox_t)

    def bands(self, d: int, det_labels, gt_labels) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        d_band, g_band = self.cset.boundary_band(d, bbox=self.d_bbox_t), self.gt.boundary_band(d)
        return self.cross(det_labels, gt_labels, d_band, g_band), d_band.area, g_band.area

    def rle_launch(self, room: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return CE.rle_counts_launch_crop(self.ops, self.cset, room, bbox=self.d_bbox_t)

    def rle_again(self) -> Tuple[np.ndarray, np.ndarray]:
        return CE.rle_counts_crop(self.ops, self.cset, bbox=self.d_bbox_t)

    def outline(self, pairs, d_px, g_px) -> OutlineAgreement:
        return self.cset.outline_agreement(self.gt, pairs, area=d_px, gt_area=g_px, bbox=self.d_bbox_t)

    def error_map(self, image, d_state, g_state, alpha: int, line: int) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.cset.error_map(self.gt, d_state, g_state, image, alpha, line, bbox=self.d_bbox_t)


def _fetch(parts: Sequence[Tuple[str, torch.Tensor]]) -> Dict[str, np.ndarray]:
    """ONE device-to-host copy of the int32 device tensors ``parts`` = ``(name, tensor)``, in that order: ``{name: host array of the
    tensor's shape}``.  A part that is absent is simply not in the list."""
    host = torch.cat([t.reshape(-1) for _, t in parts]).cpu().numpy()
    ends = np.cumsum([t.numel() for _, t in parts])
    return {name: host[end - t.numel():end].reshape(tuple(t.shape)) for (name, t), end in zip(parts, ends)}


def _score(frame: _ScoreFrame, rec: dict, det, tables: Dict[str, CE.EvalTables], to_dataset_id: Dict[int, int],
           boundary: Optional[Tuple[float, Optional[int]]] = None, report: Optional[CE.OutlineReport] = None,
           boxes_xywh: Optional[np.ndarray] = None, maps: Optional[CE.ErrorMaps] = None, image: Optional[torch.Tensor] = None) -> dict:
    """One image through the scorer, in any frame: ground truth, cross matrix, with ``boundary`` the bands, run lengths, ONE
    device-to-host copy, then the result rows and the image's rows of the IoU tables; with ``report`` the image's matched pairs are
    measured in the same frame behind that (one more copy when there is a pair).  ``det`` = the detections on the host
    (contiguous classes int64, scores float64, pixel counts int64, tight boxes ``[n, 4]`` int32).  ``boxes_xywh`` float64: the
    detections' boxes when they have regressed ones (predictor mode); default ``toBbox`` of the run lengths.  With ``maps`` (the run's
    error maps) the image's map is painted on ``image`` (uint8, on the device) in the same frame behind the table rows: one more
    copy, the picture and its counts together."""
    classes, scores64, d_area, d_bbox = det
    (H, W), anns, n = frame.hw, rec["annotations"], len(classes)
    err = frame.ground_truth(anns)
    g_cat = np.asarray([a["category_id"] for a in anns], dtype=np.int64)
    inter_t = frame.cross(classes, g_cat)
    band_t = frame.bands(CE.boundary_width(H, W, *boundary), classes, g_cat) if boundary is not None else ()
    n_t, counts_t = frame.rle_launch(CE.rle_room(d_bbox))
    host = _fetch([("n_counts", n_t), ("inter", inter_t), ("g_px", frame.gt_area)] + [("err", e) for e in err]
                  + list(zip(("band_inter", "d_band", "g_band"), band_t)) + [("counts", counts_t)])          # the ONE wait, the ONE layout
    if "err" in host:
        CE.check_rasterize_error(int(host["err"][0]))
    band = tuple(host[k].astype(np.int64) for k in ("band_inter", "d_band", "g_band")) if band_t else None
    runs = CE.rle_counts_finish(host["n_counts"], host["counts"])
    if runs is None:
        system_logger.debug(f"{rec['file_name']}: run lengths need more than {len(host['counts'])} counts; encoding again")
        runs = frame.rle_again()
    strings = CE.rle_strings(*runs)
    xywh = CE.rle_to_bbox(runs[0], runs[1], H) if boxes_xywh is None else boxes_xywh
    classes_l, xywh_l, scores_l = classes.tolist(), xywh.tolist(), scores64.tolist()
    instances = [{"image_id": rec["image_id"], "category_id": classes_l[k], "bbox": xywh_l[k], "score": scores_l[k],
                  "segmentation": {"size": [H, W], "counts": strings[k]}} for k in range(n)]
    outline = None if report is None else (report, lambda pairs, d_px, g_px: OutlineAgreement.from_host(
        frame.outline(pairs, d_px, g_px).records.cpu().numpy()))                                              # (its ONE copy)
    paint = None
    if maps is not None:
        if image is None:
            raise ValueError(f"{rec['file_name']}: the error maps need the image on the device")

        def paint(d_state, g_state):
            dst, counts = frame.error_map(image, d_state, g_state, maps.alpha, maps.line_for(H, W))
            both = torch.cat([dst.reshape(-1), counts.view(torch.uint8)]).cpu().numpy()                      # (its ONE copy)
            return both[:H * W * 3].reshape(H, W, 3), both[H * W * 3:].copy().view(np.int64)
    _add_image_rows(tables, rec, to_dataset_id, classes_l, scores64, xywh, d_area, g_cat, host["g_px"].astype(np.int64),
                    host["inter"].astype(np.int64), band, outline, maps=None if maps is None else (maps, paint))
    return {"instances": instances}


def _score_image(ops: MaskOps, rec: dict, inst, tables: Dict[str, CE.EvalTables], to_dataset_id: Dict[int, int],
                 boundary: Optional[Tuple[float, Optional[int]]] = None, report: Optional[CE.OutlineReport] = None,
                 maps: Optional[CE.ErrorMaps] = None, image: Optional[torch.Tensor] = None) -> dict:
    """Predictor mode: one image's ``Instances`` through :func:`_score` on planes.  Classes, scores, predicted boxes and the masks'
    pixel counts and tight boxes come over in one copy; the result rows and the ``bbox`` task carry the predicted boxes (float32,
    widened).  ``boundary`` / ``report`` / ``maps`` / ``image``: as for :func:`_score`."""
    H, W = int(rec["height"]), int(rec["width"])
    if tuple(inst.image_size) != (H, W):
        raise ValueError(f"{rec['file_name']}: image is {inst.image_size}, the annotation says {(H, W)}")
    if len(inst) == 0:
        frame = _PlaneFrame.empty(ops, H, W)
        det, xywh = (np.zeros((0,), np.int64), np.zeros((0,), np.float64), np.zeros((0,), np.int64), np.zeros((0, 4), np.int32)), np.zeros((0, 4), np.float32)
    else:
        packed = inst.packed_masks.contiguous()
        d_area_t, d_bbox_t = ops.area_bbox(packed)
        frame = _PlaneFrame(ops, H, W, packed, d_bbox_t)
        host = _fetch([("classes", inst.pred_classes.to(torch.int32)), ("scores", inst.scores.to(torch.float32).view(torch.int32)),
                       ("boxes", inst.pred_boxes.to(torch.float32).reshape(-1, 4).view(torch.int32)), ("area", d_area_t), ("bbox", d_bbox_t)])
        det = (host["classes"].astype(np.int64), host["scores"].view(np.float32).astype(np.float64), host["area"].astype(np.int64), host["bbox"])
        xywh = host["boxes"].view(np.float32).copy()
        xywh[:, 2] -= xywh[:, 0]
        xywh[:, 3] -= xywh[:, 1]
    return _score(frame, rec, det, tables, to_dataset_id, boundary, report, boxes_xywh=xywh.astype(np.float64), maps=maps, image=image)


def _add_image_rows(tables, rec, to_dataset_id, classes_l, scores64, d_box64, d_area, g_cat, g_px, inter, band=None, outline=None,
                    maps=None) -> None:
    """One image's rows of the tasks' tables: detections (contiguous classes, float64 scores and XYWH boxes, mask pixel
    counts) against the record's annotations (``g_px`` their rasterised pixel counts, ``inter`` the intersection counts).
    ``band`` = (band intersections, detection band areas, ground-truth band areas) fills the ``boundary`` task: its IoU is
    ``min(mask IoU, boundary IoU)``, its areas are those of ``segm``.  ``outline`` = (the run's ``OutlineReport``, the image's
    device stage): the image's pairs are matched from the ``segm`` IoU table and measured.  ``maps`` = (the run's ``ErrorMaps``, the
    image's ``paint``): the image's error map is painted from the same table and written."""
    anns = rec["annotations"]
    crowd = np.asarray([int(a.get("iscrowd", 0)) for a in anns], dtype=np.uint8)
    g_area = np.asarray([float(a["area"]) for a in anns], dtype=np.float64)
    g_box = np.asarray([_gt_box_xywh(a) for a in anns], dtype=np.float64).reshape(-1, 4)
    d_cat = np.asarray([to_dataset_id[c] for c in classes_l], dtype=np.int64)
    g_cat_ds = np.asarray([to_dataset_id[int(c)] for c in g_cat], dtype=np.int64)
    img = rec["image_id"]
    m_iou = CE.mask_iou(inter, d_area, g_px, crowd)
    tables["segm"].add_image(img, d_cat, scores64, d_area.astype(np.float64), g_cat_ds, g_area, crowd, m_iou)
    if band is not None:
        b_iou = CE.boundary_iou(band[0].reshape(m_iou.shape), band[1], band[2], crowd)
        tables["boundary"].add_image(img, d_cat, scores64, d_area.astype(np.float64), g_cat_ds, g_area, crowd, np.minimum(m_iou, b_iou))
    tables["bbox"].add_image(img, d_cat, scores64, d_box64[:, 2] * d_box64[:, 3], g_cat_ds, g_area, crowd,
                             CE.box_iou(d_box64, g_box, crowd))
    if outline is not None:
        outline[0].add_image(img, os.path.basename(str(rec["file_name"])), d_cat, scores64, d_area, g_cat_ds, g_px, crowd, m_iou, outline[1])
    if maps is not None:
        maps[0].add_image(img, str(rec["file_name"]), d_cat, scores64, g_cat_ds, crowd, m_iou, maps[1])


# ---- pipeline mode -----------------------------------------------------------------------------------------------------------
class PipelineRunner:
    """The per-image work of ``--task inference`` for the evaluate task: the models (``rcnn`` 50 / 101 = that one alone,
    ``"combo"`` = every trained one, R50 first), the settings, the small classes (``calculate_average_mask_sizes`` over the
    first <= 5 images) and the image's final instances (``final_instances``) are ``run_inference``'s own; the images of a group
    share their forwards as they do there.  ``t_read`` / ``t_pipe``: seconds spent decoding images / in the pipeline."""

    def __init__(self, dataset_name: str, metadata, split_dir: str, rcnn: Union[int, str], threshold: float):
        from ..utils.spatial_constraints import load_spatial_constraints
        from . import inference as INF

        self.INF = INF
        self.st = INF.PipelineSettings(dataset_name)
        # (what the scoring reads -- planes or the pipeline's crop set -- must be what the pipeline hands it: checked before any model is loaded)
        self.score_frame = score_frame_setting(dataset_name, self.st.mask_frame)
        predictors, models = [], []
        for r in ((50, 101) if str(rcnn) == "combo" else (int(rcnn),)):
            paths = get_trained_model_paths(split_dir, r)
            if dataset_name in paths:
                p, _ = choose_and_use_model(paths, dataset_name, threshold, metadata, r)
                if p is not None:
                    p.model.eval()
                    predictors.append(p)
                    models.append(r)
        if not predictors:
            raise FileNotFoundError(f"No trained models found for dataset '{dataset_name}' (rcnn {rcnn}) under {split_dir}")
        system_logger.info(f"Loaded models: {', '.join(f'R{r}' for r in models)}")
        self.pipe = INF.InferencePipeline(predictors, dataset_name, self.st.inf, self.st.global_config)
        if self.pipe.world != 1:
            raise RuntimeError("the evaluate task runs in one process")
        self.spatial_cfg = load_spatial_constraints(dataset_name)
        self.num_classes = len(metadata.thing_classes)
        self.dev = self.pipe.dev
        self.t_read = self.t_pipe = 0.0
        self.image_dev: Optional[torch.Tensor] = None      # the image of the instances last yielded, uint8 BGR on the device

    def _load(self, path: str) -> torch.Tensor:
        t0 = time.perf_counter()
        img = self.INF.imread_bgr(path)            # the inference task's reader (its 16-bit rule included)
        self.t_read += time.perf_counter() - t0
        if img is None:
            raise ValueError(f"Could not load image: {path}")
        return torch.from_numpy(img).to(self.dev)

    def instances(self, paths: Sequence[str]):
        """Generator over ``paths`` in order: ``(path, (H, W), packed, scores, classes, tabs)`` -- the image's final masks on the
        device (None or empty when nothing is left), its scores and classes, ``tabs = (pixel counts, boxes)`` on the host.
        ``packed`` is what ``final_instances`` keeps in the dataset's ``mask_frame``: full-frame planes ``[n, H, W/32]`` int32 under
        ``full`` (``score_frame: planes``), a :class:`CropMaskSet` under ``crop`` and ``crop_direct`` (``score_frame: crops``).
        While the consumer holds a tuple, ``image_dev`` is that image on the device (uint8 ``[H, W, 3]`` BGR): what the error maps
        are painted on."""
        INF, st, pipe = self.INF, self.st, self.pipe
        t0, r0 = time.perf_counter(), self.t_read
        on_dev = {p: self._load(p) for p in paths[:5]}
        sample = list(on_dev.items())
        if sample:
            pipe.finish_prefetch(pipe.prefetch_images(sample, [0], st.tile_size, st.overlap_ratio, st.upscale_factor))
        small_classes = INF.determine_small_classes(pipe.calculate_average_mask_sizes(sample), 50)
        system_logger.info(f"Small classes: {sorted(small_classes)}")
        models_needed = st.models_needed(len(pipe.predictors), small_classes, self.num_classes)
        tiles = len(pipe._tile_offsets(int(sample[0][1].shape[0]), int(sample[0][1].shape[1]), st.tile_size, st.overlap_ratio)) if sample else 1
        group = max(1, min(pipe.forward_batch // max(1, tiles), 16))
        phases_ok = INF.image_phases_enabled(pipe)
        del sample
        self.t_pipe += time.perf_counter() - t0 - (self.t_read - r0)
        for g0 in range(0, len(paths), group):
            t0, r0 = time.perf_counter(), self.t_read
            items = [(p, on_dev.pop(p) if p in on_dev else self._load(p)) for p in paths[g0:g0 + group]]
            pipe.finish_prefetch(pipe.prefetch_images(items, models_needed, st.tile_size, st.overlap_ratio, st.upscale_factor))
            self.t_pipe += time.perf_counter() - t0 - (self.t_read - r0)
            for path, image_dev in items:
                t0 = time.perf_counter()
                try:
                    packed, scores, classes, tabs = INF.final_instances(pipe, st, path, image_dev, small_classes, self.num_classes,
                                                                        self.spatial_cfg, phases_ok)
                finally:
                    pipe.drop_cached(path)
                self.t_pipe += time.perf_counter() - t0
                self.image_dev = image_dev
                yield path, (int(image_dev.shape[0]), int(image_dev.shape[1])), packed, scores, classes, tabs
        self.image_dev = None
        pipe.clear_cache()


def _run_pipeline(dataset_name, recs, metadata, split_dir, rcnn, threshold, tables, to_dataset_id, boundary=None, report=None, maps=None):
    """Every test image through the inference pipeline and the scorer; ``(per_image, (reads, pipeline, scoring) seconds)``."""
    system_logger.info(f"Evaluating the inference pipeline on {len(recs)} test images of {dataset_name} (rcnn {rcnn}, threshold {threshold})")
    runner = PipelineRunner(dataset_name, metadata, split_dir, rcnn, threshold)
    ops = MaskOps(str(runner.dev))
    per_image: Dict[int, dict] = {}
    t_score = 0.0
    for ri, (_, hw, packed, scores, classes, tabs) in enumerate(runner.instances([rec["file_name"] for rec in recs])):
        t0 = time.perf_counter()
        per_image[ri] = _score_pipeline_image(ops, recs[ri], hw, packed, scores, classes, tabs, tables, to_dataset_id, runner.score_frame, boundary,
                                              report, maps=maps, image=runner.image_dev if maps is not None else None)
        t_score += time.perf_counter() - t0
    return per_image, (runner.t_read, runner.t_pipe, t_score)


def _score_pipeline_image(ops: MaskOps, rec: dict, hw, packed, scores, classes, tabs, tables, to_dataset_id, score_frame: Optional[str] = None,
                          boundary: Optional[Tuple[float, Optional[int]]] = None, report: Optional[CE.OutlineReport] = None,
                          maps: Optional[CE.ErrorMaps] = None, image: Optional[torch.Tensor] = None) -> dict:
    """Pipeline mode: one image's final instances through :func:`_score`.  The detections' pixel counts and boxes are already on
    the host (``tabs``), so everything the host needs comes over in the scorer's ONE copy.  Dispatches on what ``final_instances``
    handed over: planes are scored on planes, a :class:`CropMaskSet` on rooms (``score_frame`` decides for an image that kept no
    instance).  ``boundary`` / ``report`` / ``maps`` / ``image``: as for :func:`_score`."""
    H, W = int(rec["height"]), int(rec["width"])
    if tuple(int(v) for v in hw) != (H, W):
        raise ValueError(f"{rec['file_name']}: image is {tuple(hw)}, the annotation says {(H, W)}")
    n = 0 if packed is None else int(packed.shape[0])
    if n == 0:
        d_area, d_bbox = np.zeros((0,), np.int64), np.zeros((0, 4), np.int32)
    else:
        d_area, d_bbox = np.asarray(tabs[0]).astype(np.int64), np.ascontiguousarray(np.asarray(tabs[1]).reshape(-1, 4), dtype=np.int32)
    det = (np.asarray([int(c) for c in classes][:n], dtype=np.int64), np.asarray([float(v) for v in scores][:n], dtype=np.float64), d_area, d_bbox)
    if isinstance(packed, CropMaskSet) or (n == 0 and score_frame == "crops"):
        frame = _CropFrame(ops, packed, ops.upload(d_bbox)) if n else _CropFrame.empty(ops, H, W)
    else:
        ops.set_frame_width(W)
        frame = _PlaneFrame(ops, H, W, packed.contiguous(), torch.from_numpy(d_bbox).to(ops.device)) if n else _PlaneFrame.empty(ops, H, W)
    return _score(frame, rec, det, tables, to_dataset_id, boundary, report, maps=maps, image=image)
