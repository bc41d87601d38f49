"""``main.py --task evaluate``: COCO box and mask AP of a trained model on the dataset's test split.

What the reference's user guide describes (docs/user-guide.md, "Model Evaluation") with Detectron2's ``COCOEvaluator`` +
``inference_on_dataset`` semantics (the reference's own ``evaluate_model.py`` cannot run as written: it passes ``rcnn`` in
the ``metadata`` slot of ``choose_and_use_model``).  Every test image goes through the whole-image predictor (800 / 1333
resize, score threshold 0.45, at most 100 detections); the ground truth is rasterised, intersected with the detections and
run-length encoded on the GPU (``deepemia_amd.cocoeval``), and COCOeval's matching runs as one native host call.

Outputs in ``output_dir``: ``metrics.csv`` (``metric,value``, one row per task), ``coco_instances_results.json``
(``instances_to_coco_json`` layout, dataset category ids) and ``instances_predictions.pth``.  Not provided: prediction
images (``--visualize`` only logs a warning) and the ``combo`` model pair.
"""
from __future__ import annotations

import csv
import json
import os
import time
from collections import OrderedDict
from pathlib import Path
from typing import Dict, List

import numpy as np
import torch

from .. import cocoeval as CE
from ..data.datasets import (MetadataCatalog, get_split_dicts, load_coco_test, load_or_create_split, read_dataset_info,
                             register_datasets, rle_counts_of)
from ..data.models import choose_and_use_model, get_trained_model_paths
from ..maskset import MaskOps
from ..utils.config import get_config
from ..utils.logger_utils import system_logger

SCORE_THRESH = 0.45          # evaluate_model.py:78 (--threshold does not apply)
BATCH = 4                    # same-size test images per forward


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


def _gt_box_xywh(a: dict) -> List[float]:
    """``convert_to_coco_dict``'s box: XYWH, each value ``round(float(x), 3)``."""
    b = [float(v) for v in a["bbox"]]
    if a.get("bbox_mode", "XYXY_ABS") == "XYXY_ABS":
        b = [b[0], b[1], b[2] - b[0], b[3] - b[1]]
    return [round(v, 3) for v in b]


def evaluate_model(dataset_name: str, output_dir: str, visualize: bool = False, dataset_format: str = "json",
                   rcnn: int = 101) -> "OrderedDict[str, Dict[str, float]]":
    """Score the trained ``rcnn_r<rcnn>`` model of ``dataset_name`` on its test split; returns Detectron2's
    ``OrderedDict(bbox={...}, segm={...})`` and writes the three result files to ``output_dir``."""
    t_start = time.perf_counter()
    config = get_config()
    split_dir = Path(config["paths"]["split_dir"]).expanduser().resolve()
    category_json = Path(config["paths"]["category_json"]).expanduser().resolve()
    if visualize:
        system_logger.warning("--visualize: evaluation images are not drawn in this build (Detectron2's Visualizer is not "
                              "provided); the metrics are computed as usual")
    dataset_info = read_dataset_info(category_json)
    register_datasets(dataset_info, dataset_name, dataset_format=dataset_format)
    recs, class_names, to_dataset_id = _test_records(dataset_name, dataset_format, dataset_info, split_dir)
    metadata = MetadataCatalog.get(f"{dataset_name}_train")
    predictor, _ = choose_and_use_model(get_trained_model_paths(str(split_dir), rcnn), dataset_name, SCORE_THRESH, metadata, rcnn)
    if predictor is None:
        raise FileNotFoundError(f"no trained rcnn_r{rcnn} model for dataset {dataset_name} under {split_dir}")
    device = predictor.engine.device
    ops = MaskOps(str(device))
    system_logger.info(f"Evaluating {len(recs)} test images of {dataset_name} (R{rcnn}, score threshold {SCORE_THRESH})")

    t_read = t_fwd = t_score = 0.0
    tables = {"bbox": CE.EvalTables(), "segm": CE.EvalTables()}
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
            per_image[ri] = _score_image(ops, recs[ri], out["instances"], tables, to_dataset_id)
        t3 = time.perf_counter()
        t_read += t1 - t0
        t_fwd += t2 - t1
        t_score += t3 - t2

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
        for task in ("bbox", "segm"):
            results[task] = {m: float("nan") for m in CE.METRICS}
    else:
        ev = CE.evaluate(tables, [r["image_id"] for r in recs], cat_ids)
        for task in ("bbox", "segm"):
            system_logger.info(f"Evaluation results for {task}:\n" + "\n".join(CE.summary_lines(ev[task]["stats"])))
            results[task] = CE.derive_results(ev[task]["stats"], ev[task]["precision"], class_names)
    t_score += time.perf_counter() - t0
    system_logger.info(f"Evaluation metrics: {results}")
    csv_path = Path(output_dir) / "metrics.csv"
    with open(csv_path, mode="w", newline="") as f:
        w = csv.DictWriter(f, fieldnames=["metric", "value"])
        w.writeheader()
        for key, value in results.items():
            w.writerow({"metric": key, "value": value})
    n = max(1, len(recs))
    system_logger.info(f"Evaluation wall time {time.perf_counter() - t_start:.2f}s: forwards {t_fwd:.3f}s ({1e3 * t_fwd / n:.1f} ms/image), "
                       f"scoring {t_score:.3f}s ({1e3 * t_score / n:.1f} ms/image), image reads {t_read:.3f}s; "
                       f"metrics saved to {csv_path}")
    return results


def _score_image(ops: MaskOps, rec: dict, inst, tables: Dict[str, CE.EvalTables], to_dataset_id: Dict[int, int]) -> dict:
    """Device work of one image (ground-truth masks, intersections, run lengths) and its rows of the IoU tables."""
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
    counts, off = CE.rle_counts(ops, packed, d_bbox_t, W)
    strings = CE.rle_strings(counts, off)
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
    crowd = np.asarray([int(a.get("iscrowd", 0)) for a in anns], dtype=np.uint8)
    g_area = np.asarray([float(a["area"]) for a in anns], dtype=np.float64)
    g_box = np.asarray([_gt_box_xywh(a) for a in anns], dtype=np.float64).reshape(-1, 4)
    d_cat = np.asarray([to_dataset_id[c] for c in classes_l], dtype=np.int64)
    g_cat_ds = np.asarray([to_dataset_id[int(c)] for c in g_cat], dtype=np.int64)
    d_box64 = xywh.astype(np.float64)
    img = rec["image_id"]
    tables["segm"].add_image(img, d_cat, scores.astype(np.float64), d_area.astype(np.float64), g_cat_ds, g_area, crowd,
                             CE.mask_iou(inter, d_area, g_px, crowd))
    tables["bbox"].add_image(img, d_cat, scores.astype(np.float64), d_box64[:, 2] * d_box64[:, 3], g_cat_ds, g_area, crowd,
                             CE.box_iou(d_box64, g_box, crowd))
    return {"instances": instances}
