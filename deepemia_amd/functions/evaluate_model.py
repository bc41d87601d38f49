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

Outputs in ``output_dir``: ``metrics.csv`` (``metric,value``, one row per task: ``bbox``, ``segm`` and, when asked for, ``boundary``), ``coco_instances_results.json``
(``instances_to_coco_json`` layout, dataset category ids) and ``instances_predictions.pth``; with the outline report,
``outline_agreement.csv`` (one row per matched pair, in image order, then detection order) and ``outline_summary.csv`` (one row per
class and the row ``all``, pooled over the pairs; a class without a pair has empty value fields).  Not provided: prediction
images (``--visualize`` only logs a warning) and, in predictor mode, the ``combo`` model pair.
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


def evaluation_settings(dataset_name: Optional[str] = None) -> Tuple[str, List[int]]:
    """``(mode, max_dets)`` from the ``evaluation`` key of the configuration (global, or in the dataset's file; neither entry is
    required); ``DEEPEMIA_EVAL_MODE`` overrides the mode.  ValueError for an unknown mode or a malformed ``max_dets``."""
    try:
        cfg = (get_config(dataset_name=dataset_name) if dataset_name else get_config()).get("evaluation", {}) or {}
    except FileNotFoundError:        # (no configuration at all: the caller's own read reports it)
        cfg = {}
    mode = str(os.environ.get("DEEPEMIA_EVAL_MODE") or cfg.get("mode", "predictor")).strip().lower()
    if mode not in MODES:
        raise ValueError(f"evaluation mode must be one of {MODES}, got {mode!r}")
    return mode, CE.check_max_dets(cfg.get("max_dets"))


def score_frame_setting(dataset_name: Optional[str] = None, mask_frame: Optional[str] = None) -> str:
    """``evaluation.score_frame`` (global, or in the dataset's file, next to ``mode`` and ``max_dets``): what the pipeline mode's
    scoring reads, ``planes`` (the default) or ``crops``; the predictor mode never asks.  ValueError for an unknown value and,
    when the dataset's ``mask_frame`` is given, for a pair that does not go together: ``crops`` scores the pipeline's
    :class:`CropMaskSet` and needs ``mask_frame: crop`` or ``crop_direct``; ``planes`` scores planes and needs ``mask_frame: full``."""
    try:
        cfg = (get_config(dataset_name=dataset_name) if dataset_name else get_config()).get("evaluation", {}) or {}
    except FileNotFoundError:        # (no configuration at all: the caller's own read reports it)
        cfg = {}
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
    try:
        cfg = (get_config(dataset_name=dataset_name) if dataset_name else get_config()).get("evaluation", {}) or {}
    except FileNotFoundError:        # (no configuration at all: the caller's own read reports it)
        cfg = {}
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
    try:
        cfg = (get_config(dataset_name=dataset_name) if dataset_name else get_config()).get("evaluation", {}) or {}
    except FileNotFoundError:        # (no configuration at all: the caller's own read reports it)
        cfg = {}
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


def _gt_masks(ops: MaskOps, anns: List[dict], H: int, W: int):
    """Packed ground-truth masks of one image in annotation order, pixel counts and boxes (device)."""
    poly_idx = [i for i, a in enumerate(anns) if isinstance(a.get("segmentation"), list)]
    rle_idx = [i for i, a in enumerate(anns) if isinstance(a.get("segmentation"), dict)]
    if any(a.get("segmentation") is None for a in anns):
        raise ValueError("ground truth without a segmentation cannot be scored for masks")
    packed, area, bbox = CE.rasterize_polygons(ops, [anns[i]["segmentation"] for i in poly_idx], H, W)
    if not rle_idx:
        return packed, area, bbox
    dense = np.stack([CE.rle_decode(rle_counts_of(anns[i]["segmentation"]), H, W) for i in rle_idx])
    allm = torch.empty((len(anns), H, (W + 31) // 32), dtype=torch.int32, device=ops.device)
    if poly_idx:
        allm[torch.tensor(poly_idx, device=ops.device)] = packed
    allm[torch.tensor(rle_idx, device=ops.device)] = ops.from_dense(dense)
    area, bbox = ops.area_bbox(allm)
    return allm, area, bbox


def _gt_crops(ops: MaskOps, anns: List[dict], H: int, W: int) -> Tuple[CropMaskSet, torch.Tensor]:
    """The ground truth of one image as a :class:`CropMaskSet` in annotation order (its ``area`` / ``bbox``: pixel counts and
    boxes on the device) and the rasteriser's error word: polygons are rasterised into rooms, run-length annotations are packed
    on the host.  Nothing is waited for."""
    if any(a.get("segmentation") is None for a in anns):
        raise ValueError("ground truth without a segmentation cannot be scored for masks")
    poly_idx = [i for i, a in enumerate(anns) if isinstance(a.get("segmentation"), list)]
    rle_idx = [i for i, a in enumerate(anns) if isinstance(a.get("segmentation"), dict)]
    polys, err = CE.rasterize_polygons_crop(ops, [anns[i]["segmentation"] for i in poly_idx], H, W)
    if not rle_idx:
        return polys, err
    runs = CE.rle_crop_set(ops, [rle_counts_of(anns[i]["segmentation"]) for i in rle_idx], H, W)
    if not poly_idx:
        return runs, err
    place = np.empty(len(anns), dtype=np.int64)
    place[poly_idx + rle_idx] = np.arange(len(anns))
    return CropMaskSet.cat([polys, runs]).select(place), err


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
    config = get_config()
    max_dets = CE.check_max_dets((get_config(dataset_name=dataset_name).get("evaluation", {}) or {}).get("max_dets"))
    split_dir = Path(config["paths"]["split_dir"]).expanduser().resolve()
    category_json = Path(config["paths"]["category_json"]).expanduser().resolve()
    if visualize:
        system_logger.warning("--visualize: evaluation images are not drawn in this build (Detectron2's Visualizer is not "
                              "provided); the metrics are computed as usual")
    dataset_info = read_dataset_info(category_json)
    register_datasets(dataset_info, dataset_name, dataset_format=dataset_format)
    recs, class_names, to_dataset_id = _test_records(dataset_name, dataset_format, dataset_info, split_dir)
    metadata = MetadataCatalog.get(f"{dataset_name}_train")
    if mode == "pipeline":
        tables = _new_tables(boundary)
        per_image, times = _run_pipeline(dataset_name, recs, metadata, str(split_dir), rcnn, threshold, tables, to_dataset_id, boundary, report)
        return _write_results(recs, per_image, tables, to_dataset_id, class_names, output_dir, max_dets, t_start, times, "pipeline", report)
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
        for ri, out in zip(group, outs):
            per_image[ri] = _score_image(ops, recs[ri], out["instances"], tables, to_dataset_id, boundary, report)
        t3 = time.perf_counter()
        t_read += t1 - t0
        t_fwd += t2 - t1
        t_score += t3 - t2

    return _write_results(recs, per_image, tables, to_dataset_id, class_names, output_dir, max_dets, t_start, (t_read, t_fwd, t_score),
                          "forwards", report)


def _new_tables(boundary=None) -> Dict[str, CE.EvalTables]:
    """The tasks' tables in the order of the results: ``bbox``, ``segm`` and, with the boundary-AP switch on, ``boundary``."""
    tables = {"bbox": CE.EvalTables(), "segm": CE.EvalTables()}
    if boundary is not None:
        tables["boundary"] = CE.EvalTables()
    return tables


def _write_results(recs, per_image, tables, to_dataset_id, class_names, output_dir, max_dets, t_start, times, work: str,
                   report: Optional[CE.OutlineReport] = None):
    """COCOeval over the tables of all images, the three result files and the timing line (``work`` names what ``times[1]``
    measured: the predictor's forwards, or the whole inference pipeline of an image).  ``report``: the run's outline-agreement
    report, when asked for -- its two files are written beside the three and its ``all`` row is logged."""
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
    n = max(1, len(recs))
    system_logger.info(f"Evaluation wall time {time.perf_counter() - t_start:.2f}s: {work} {t_fwd:.3f}s ({1e3 * t_fwd / n:.1f} ms/image), "
                       f"scoring {t_score:.3f}s ({1e3 * t_score / n:.1f} ms/image), image reads {t_read:.3f}s; "
                       f"metrics saved to {csv_path}")
    return results


def _score_image(ops: MaskOps, rec: dict, inst, tables: Dict[str, CE.EvalTables], to_dataset_id: Dict[int, int],
                 boundary: Optional[Tuple[float, Optional[int]]] = None, report: Optional[CE.OutlineReport] = None) -> dict:
    """Device work of one image (ground-truth masks, intersections, run lengths) and its rows of the IoU tables.  ``boundary``:
    :func:`boundary_setting`'s value; not None adds the bands of both sides and their intersections for the ``boundary`` task.
    ``report``: the run's outline-agreement report; not None measures the image's matched pairs behind the copies (one more)."""
    H, W = int(rec["height"]), int(rec["width"])
    if tuple(inst.image_size) != (H, W):
        raise ValueError(f"{rec['file_name']}: image is {inst.image_size}, the annotation says {(H, W)}")
    anns = rec["annotations"]
    n = len(inst)
    packed = inst.packed_masks if n else torch.zeros((0, H, (W + 31) // 32), dtype=torch.int32, device=ops.device)
    packed = packed.contiguous()
    d_area_t, d_bbox_t = ops.area_bbox(packed)
    g_packed, g_area_t, g_bbox_t = _gt_masks(ops, anns, H, W)
    classes = inst.pred_classes.cpu().numpy().astype(np.int64) if n else np.zeros((0,), np.int64)
    g_cat = np.asarray([a["category_id"] for a in anns], dtype=np.int64)
    inter_t = CE.cross_matrix(ops, packed, d_bbox_t, classes, g_packed, g_bbox_t, g_cat, W)
    band_t = _plane_bands(ops, boundary, H, W, packed, d_bbox_t, classes, g_packed, g_bbox_t, g_cat)
    counts, off = CE.rle_counts(ops, packed, d_bbox_t, W)
    strings = CE.rle_strings(counts, off)
    band = tuple(t.cpu().numpy().astype(np.int64) for t in band_t) if band_t else None
    inter = inter_t.cpu().numpy().astype(np.int64)
    d_area = d_area_t.cpu().numpy().astype(np.int64)
    g_px = g_area_t.cpu().numpy().astype(np.int64)
    boxes = inst.pred_boxes.cpu().numpy().astype(np.float32).reshape(-1, 4) if n else np.zeros((0, 4), np.float32)
    scores = inst.scores.cpu().numpy().astype(np.float32) if n else np.zeros((0,), np.float32)
    xywh = boxes.copy()
    xywh[:, 2] -= xywh[:, 0]
    xywh[:, 3] -= xywh[:, 1]
    xywh_l, scores_l, classes_l = xywh.tolist(), scores.tolist(), classes.tolist()
    instances = [{"image_id": rec["image_id"], "category_id": classes_l[k], "bbox": xywh_l[k], "score": scores_l[k],
                  "segmentation": {"size": [H, W], "counts": strings[k]}} for k in range(n)]
    outline = None if report is None else (report, _outline_stage(
        lambda pairs, da, ga: ops.outline_agreement(packed, d_bbox_t, da, g_packed, g_bbox_t, ga, pairs, W=W)))
    _add_image_rows(tables, rec, to_dataset_id, classes_l, scores.astype(np.float64), xywh.astype(np.float64), d_area, g_cat, g_px, inter, band,
                    outline)
    return {"instances": instances}


def _outline_stage(launch):
    """The device stage of the outline report for one image, as ``OutlineReport.add_image`` calls it when the image has a pair:
    ``launch(pairs, detection pixel counts, annotation pixel counts)`` enqueues the kernels on the frame being scored, and the
    records come over in ONE copy."""
    return lambda pairs, d_px, g_px: OutlineAgreement.from_host(launch(pairs, d_px, g_px).records.cpu().numpy())


def _plane_bands(ops: MaskOps, boundary, H: int, W: int, packed, d_bbox_t, classes, g_packed, g_bbox_t, g_cat):
    """The boundary task's device work on planes, enqueued without a wait: the bands of the detections and of the rasterised ground
    truth at the image's width ``d`` and their cross matrix -- ``(band intersections [n, G], detection band areas [n], ground-truth
    band areas [G])`` int32 on the device, or None with the switch off."""
    if boundary is None:
        return None
    d = CE.boundary_width(H, W, *boundary)
    d_band, d_ba = ops.boundary_band(packed, d_bbox_t, d, W)
    g_band, g_ba = ops.boundary_band(g_packed, g_bbox_t, d, W)
    return CE.cross_matrix(ops, d_band, d_bbox_t, classes, g_band, g_bbox_t, g_cat, W), d_ba, g_ba


def _add_image_rows(tables, rec, to_dataset_id, classes_l, scores64, d_box64, d_area, g_cat, g_px, inter, band=None, outline=None) -> None:
    """One image's rows of the tasks' tables: detections (contiguous classes, float64 scores and XYWH boxes, mask pixel
    counts) against the record's annotations (``g_px`` their rasterised pixel counts, ``inter`` the intersection counts).
    ``band`` = (band intersections, detection band areas, ground-truth band areas) fills the ``boundary`` task: its IoU is
    ``min(mask IoU, boundary IoU)``, its areas are those of ``segm``.  ``outline`` = (the run's ``OutlineReport``, the image's
    device stage): the image's pairs are matched from the ``segm`` IoU table and measured."""
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
        ``full`` (``score_frame: planes``), a :class:`CropMaskSet` under ``crop`` and ``crop_direct`` (``score_frame: crops``)."""
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
                yield path, (int(image_dev.shape[0]), int(image_dev.shape[1])), packed, scores, classes, tabs
        pipe.clear_cache()


def _run_pipeline(dataset_name, recs, metadata, split_dir, rcnn, threshold, tables, to_dataset_id, boundary=None, report=None):
    """Every test image through the inference pipeline and the scorer; ``(per_image, (reads, pipeline, scoring) seconds)``."""
    system_logger.info(f"Evaluating the inference pipeline on {len(recs)} test images of {dataset_name} (rcnn {rcnn}, threshold {threshold})")
    runner = PipelineRunner(dataset_name, metadata, split_dir, rcnn, threshold)
    ops = MaskOps(str(runner.dev))
    per_image: Dict[int, dict] = {}
    t_score = 0.0
    for ri, (_, hw, packed, scores, classes, tabs) in enumerate(runner.instances([rec["file_name"] for rec in recs])):
        t0 = time.perf_counter()
        per_image[ri] = _score_pipeline_image(ops, recs[ri], hw, packed, scores, classes, tabs, tables, to_dataset_id, runner.score_frame, boundary,
                                              report)
        t_score += time.perf_counter() - t0
    return per_image, (runner.t_read, runner.t_pipe, t_score)


def _score_pipeline_image(ops: MaskOps, rec: dict, hw, packed, scores, classes, tabs, tables, to_dataset_id, score_frame: Optional[str] = None,
                          boundary: Optional[Tuple[float, Optional[int]]] = None, report: Optional[CE.OutlineReport] = None) -> dict:
    """Device work of one image's final instances (ground-truth masks, intersections, run lengths) and its rows of the IoU
    tables.  Everything the host needs comes over in ONE device-to-host copy; the detections' pixel counts and boxes are
    already on the host (``tabs``).  Dispatches on what ``final_instances`` handed over: planes are scored on planes, a
    :class:`CropMaskSet` on rooms (``score_frame`` decides for an image that kept no instance).  ``boundary``:
    :func:`boundary_setting`'s value; not None adds the band launches, and their counts ride the same copy.  ``report``: the run's
    outline-agreement report; not None matches the image's pairs from that copy and, where there is one, measures them in the
    frame being scored -- exactly one more copy."""
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
        return _score_crops(ops, rec, H, W, packed if n else CropMaskSet.empty(ops, (H, W)), det, tables, to_dataset_id, boundary, report)
    if n == 0:
        packed = torch.zeros((0, H, (W + 31) // 32), dtype=torch.int32, device=ops.device)
    return _score_planes(ops, rec, H, W, packed.contiguous(), det, tables, to_dataset_id, boundary, report)


def _score_planes(ops: MaskOps, rec: dict, H: int, W: int, packed: torch.Tensor, det, tables, to_dataset_id, boundary=None, report=None) -> dict:
    """``score_frame: planes``: the detections are full-frame planes and every annotation is rasterised into one."""
    anns = rec["annotations"]
    classes, _, _, d_bbox = det
    ops.set_frame_width(W)
    d_bbox_t = torch.from_numpy(d_bbox).to(ops.device)
    if any(isinstance(a.get("segmentation"), dict) for a in anns):
        g_packed, g_area_t, g_bbox_t = _gt_masks(ops, anns, H, W)          # (RLE ground truth: its own waits)
        err = []
    else:
        if any(a.get("segmentation") is None for a in anns):
            raise ValueError("ground truth without a segmentation cannot be scored for masks")
        err = []
        g_packed, g_area_t, g_bbox_t = CE.rasterize_polygons(ops, [a["segmentation"] for a in anns], H, W, err_out=err)
    g_cat = np.asarray([a["category_id"] for a in anns], dtype=np.int64)
    inter_t = CE.cross_matrix(ops, packed, d_bbox_t, classes, g_packed, g_bbox_t, g_cat, W)
    band_t = _plane_bands(ops, boundary, H, W, packed, d_bbox_t, classes, g_packed, g_bbox_t, g_cat)
    n_t, counts_t = CE.rle_counts_launch(ops, packed, d_bbox_t, W, CE.rle_room(d_bbox))
    host = torch.cat([n_t, inter_t.reshape(-1), g_area_t.reshape(-1)] + [e.reshape(-1) for e in err] + [t.reshape(-1) for t in band_t or ()]
                     + [counts_t]).cpu().numpy()                                                                                    # the ONE wait
    outline = None if report is None else (report, _outline_stage(
        lambda pairs, da, ga: ops.outline_agreement(packed, d_bbox_t, da, g_packed, g_bbox_t, ga, pairs, W=W)))
    return _finish_pipeline_image(rec, H, det, g_cat, host, bool(err), int(counts_t.shape[0]), tables, to_dataset_id,
                                  lambda: CE.rle_counts(ops, packed, d_bbox_t, W), band_t is not None, outline)


def _score_crops(ops: MaskOps, rec: dict, H: int, W: int, cset: CropMaskSet, det, tables, to_dataset_id, boundary=None, report=None) -> dict:
    """``score_frame: crops``: the same launches over rooms -- the ground truth becomes a :class:`CropMaskSet` too, the cross
    matrix and the run lengths read both sets' words in place, and the bands of the boundary task are sets over the same rooms.
    No ``[*, H, W/32]`` tensor exists here."""
    anns = rec["annotations"]
    classes, _, _, d_bbox = det
    d_bbox_t = ops.upload(d_bbox) if len(cset) else cset.bbox
    gt, err = _gt_crops(ops, anns, H, W)
    g_cat = np.asarray([a["category_id"] for a in anns], dtype=np.int64)
    inter_t = CE.cross_matrix_crop(ops, cset, classes, gt, g_cat, det_bbox=d_bbox_t)
    band_t = []
    if boundary is not None:
        d = CE.boundary_width(H, W, *boundary)
        d_band, g_band = cset.boundary_band(d, bbox=d_bbox_t), gt.boundary_band(d)
        band_t = [CE.cross_matrix_crop(ops, d_band, classes, g_band, g_cat, det_bbox=d_bbox_t).reshape(-1), d_band.area, g_band.area]
    n_t, counts_t = CE.rle_counts_launch_crop(ops, cset, CE.rle_room(d_bbox), bbox=d_bbox_t)
    host = torch.cat([n_t, inter_t.reshape(-1), gt.area.reshape(-1), err.reshape(-1)] + band_t + [counts_t]).cpu().numpy()           # the ONE wait
    outline = None if report is None else (report, _outline_stage(
        lambda pairs, da, ga: cset.outline_agreement(gt, pairs, area=da, gt_area=ga, bbox=d_bbox_t)))
    return _finish_pipeline_image(rec, H, det, g_cat, host, True, int(counts_t.shape[0]), tables, to_dataset_id,
                                  lambda: CE.rle_counts_crop(ops, cset, bbox=d_bbox_t), boundary is not None, outline)


def _finish_pipeline_image(rec: dict, H: int, det, g_cat, host: np.ndarray, has_err: bool, room: int, tables, to_dataset_id, encode_again,
                           has_band: bool = False, outline=None) -> dict:
    """Host side of both scorers, from the one copy ``host`` = run-length sizes [n], intersections [n, G], ground-truth pixel
    counts [G], the rasteriser's error word (``has_err``), with ``has_band`` the band intersections [n, G] and the band areas of
    the detections [n] and of the ground truth [G], the run-length room: the result rows and the image's rows of the IoU
    tables.  ``encode_again`` runs the two-pass encoder (one more wait) when the room was too small.  ``outline``: as for
    :func:`_add_image_rows`."""
    classes, scores64, d_area, _ = det
    n, G, W = len(classes), len(g_cat), int(rec["width"])
    classes_l = classes.tolist()
    n_host, pos = host[:n], n
    inter = host[pos:pos + n * G].reshape(n, G).astype(np.int64)
    pos += n * G
    g_px = host[pos:pos + G].astype(np.int64)
    pos += G
    if has_err:
        CE.check_rasterize_error(int(host[pos]))
        pos += 1
    band = None
    if has_band:
        band = (host[pos:pos + n * G].reshape(n, G).astype(np.int64), host[pos + n * G:pos + n * G + n].astype(np.int64),
                host[pos + n * G + n:pos + n * G + n + G].astype(np.int64))
        pos += n * G + n + G
    runs = CE.rle_counts_finish(n_host, host[pos:pos + room]) if n else (np.zeros((0,), np.uint32), np.zeros((1,), np.int64))
    if runs is None:
        system_logger.debug(f"{rec['file_name']}: run lengths need more than {room} counts; encoding again")
        runs = encode_again()
    strings = CE.rle_strings(*runs)
    xywh = CE.rle_to_bbox(runs[0], runs[1], H)
    xywh_l, scores_l = xywh.tolist(), scores64.tolist()
    instances = [{"image_id": rec["image_id"], "category_id": classes_l[k], "bbox": xywh_l[k], "score": scores_l[k],
                  "segmentation": {"size": [H, W], "counts": strings[k]}} for k in range(n)]
    _add_image_rows(tables, rec, to_dataset_id, classes_l, scores64, xywh, d_area, g_cat, g_px, inter, band, outline)
    return {"instances": instances}
