"""An independent reference for RPN proposal selection (``demia_rpn_proposals``): Detectron2 0.6
``RPN.predict_proposals`` / ``find_top_rpn_proposals`` with torchvision's hard NMS, restated in plain numpy from the
contract in ``include/deepemia_hip.h``.  No GPU, no import from the project, and none of the kernel's structure: no
histogram, no radix, no bit matrix -- one ``lexsort`` per level, a float64 decode, a greedy loop, one ``lexsort`` to merge.

Per image:
  * SELECTION, per level: all ``H W 3`` logits ordered by (value descending, flattened (h, w, a) index ascending), the
    first ``min(total, pre_topk)`` taken.  Values compare as IEEE numbers, so -0.0 and +0.0 tie (lower index first), and a
    NaN sorts above everything, as in ``torch.sort(descending=True)``.  (Upstream's ``topk`` leaves the order of equal
    values open; the project's header fixes "lower index first".  Whether -0.0 ties with +0.0 is NOT stated there: the case
    table keeps every +0.0 at a lower index than every -0.0 of its level and both off the cut, where either reading gives
    the same order.  NaNs of one level all carry one payload.)
  * DECODE in float64 from the float32 inputs: anchor = (w, h) * stride + cell; weights 1, 1, 1, 1; size deltas clamped at
    ``log(1000 / 16)`` with torch semantics (``np.minimum``: NaN stays NaN).  A row is dropped when a coordinate BEFORE
    clipping, or its score, is not finite; then clipped to ``[0, img_w] x [0, img_h]``; then dropped unless
    ``x2 - x1 > 0`` and ``y2 - y1 > 0``.
  * NMS per level: greedy, in selection order, IoU in float64 with ``area = (x2 - x1)(y2 - y1)``, suppress when
    ``IoU > thresh``.  Dropped rows take no part.
  * MERGE: the survivors of all levels by (score descending, level ascending, rank in level ascending), the first
    ``post_topk`` kept.

Besides the outputs every call returns how close its decisions were (``margins``) and why rows were dropped
(``dropped``): ``tests/test_cpu_rpn_select_ref.py`` holds the case table to a minimum margin, so that no decision of the
table can depend on float32 against float64 rounding.

``mutant`` switches ONE deliberate mistake on (the CPU test shows that the case table notices each of them).
"""
import math

import numpy as np

SCALE_CLAMP = math.log(1000.0 / 16)
MUTANTS = ("tie_order_reversed", "nms_greater_equal", "nms_across_levels", "clip_before_finite_test", "no_clamp",
           "pre_topk_off_by_one", "merge_by_level")


def select(logits: np.ndarray, pre_topk: int, mutant=None) -> np.ndarray:
    """Indices of the first ``min(total, pre_topk)`` of ``logits`` (1-D float32) by (value descending, index ascending)."""
    total = logits.shape[0]
    idx = np.arange(total)
    isnan = np.isnan(logits)
    v = np.where(isnan, np.float32(0), logits).astype(np.float64)
    tie = -idx if mutant == "tie_order_reversed" else idx
    order = np.lexsort((tie, -v, ~isnan))            # last key first: NaN rows, then value descending, then index
    k = min(total, pre_topk)
    if mutant == "pre_topk_off_by_one":
        k = min(total, pre_topk + 1)
    return order[:k]


def decode(deltas: np.ndarray, hh: np.ndarray, ww: np.ndarray, aa: np.ndarray, cell: np.ndarray, stride: int, mutant=None):
    """Float64 boxes [k, 4] BEFORE clipping of the anchors (hh, ww, aa) of one level with their float32 ``deltas`` [k, 4], and
    the scale ``S`` [k, 2] (x, y) of the arithmetic: |centre| + |d size| + exp(dsize) size, which bounds every intermediate."""
    c = cell.astype(np.float64)[aa]                                            # [k, 4]
    sx, sy = (ww * stride).astype(np.float64), (hh * stride).astype(np.float64)
    ax1, ay1, ax2, ay2 = sx + c[:, 0], sy + c[:, 1], sx + c[:, 2], sy + c[:, 3]
    wd, ht = ax2 - ax1, ay2 - ay1
    cx, cy = ax1 + 0.5 * wd, ay1 + 0.5 * ht
    d = deltas.astype(np.float64)
    with np.errstate(all="ignore"):
        dw, dh = d[:, 2], d[:, 3]
        if mutant != "no_clamp":
            dw, dh = np.minimum(dw, SCALE_CLAMP), np.minimum(dh, SCALE_CLAMP)   # np.minimum propagates NaN, as torch.clamp does
        pcx, pcy = d[:, 0] * wd + cx, d[:, 1] * ht + cy
        pw, ph = np.exp(dw) * wd, np.exp(dh) * ht
        box = np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw, pcy + 0.5 * ph], axis=1)
        S = np.stack([np.abs(cx) + np.abs(d[:, 0] * wd) + pw, np.abs(cy) + np.abs(d[:, 1] * ht) + ph], axis=1)
    return box, S


def decode_f32(deltas: np.ndarray, hh, ww, aa, cell: np.ndarray, stride: int) -> np.ndarray:
    """The same decode in float32 with one rounding per operation (separate multiply and add, no FMA) in the order a
    float32 implementation of Detectron2's ``apply_deltas`` takes: the measure of what float32 costs against ``decode``."""
    f = np.float32
    c = cell.astype(f)[aa]
    sx, sy = (ww * stride).astype(f), (hh * stride).astype(f)
    ax1, ay1, ax2, ay2 = sx + c[:, 0], sy + c[:, 1], sx + c[:, 2], sy + c[:, 3]
    wd, ht = ax2 - ax1, ay2 - ay1
    cx, cy = ax1 + f(0.5) * wd, ay1 + f(0.5) * ht
    d = deltas.astype(f)
    with np.errstate(all="ignore"):
        dw, dh = np.minimum(d[:, 2], f(SCALE_CLAMP)), np.minimum(d[:, 3], f(SCALE_CLAMP))
        pcx, pcy = d[:, 0] * wd + cx, d[:, 1] * ht + cy
        pw, ph = np.exp(dw) * wd, np.exp(dh) * ht
        out = np.stack([pcx - f(0.5) * pw, pcy - f(0.5) * ph, pcx + f(0.5) * pw, pcy + f(0.5) * ph], axis=1)
    assert out.dtype == f
    return out


def clip(box: np.ndarray, img_h: int, img_w: int) -> np.ndarray:
    out = box.copy()
    with np.errstate(all="ignore"):
        out[:, 0::2] = np.clip(box[:, 0::2], 0.0, float(img_w))
        out[:, 1::2] = np.clip(box[:, 1::2], 0.0, float(img_h))
    return out


def _greedy(boxes: np.ndarray, group: np.ndarray, thresh: float, margins: dict, mutant=None) -> np.ndarray:
    """Greedy hard NMS of ``boxes`` [m, 4] in the given order; rows of different ``group`` never meet.  Returns the kept mask."""
    m = boxes.shape[0]
    alive = np.ones(m, dtype=bool)
    kept = np.zeros(m, dtype=bool)
    area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    for i in range(m):
        if not alive[i]:
            continue
        kept[i] = True
        j = np.nonzero(alive[i + 1:] & (group[i + 1:] == group[i]))[0] + i + 1
        if j.size == 0:
            continue
        b = boxes[j]
        w = np.maximum(0.0, np.minimum(boxes[i, 2], b[:, 2]) - np.maximum(boxes[i, 0], b[:, 0]))
        h = np.maximum(0.0, np.minimum(boxes[i, 3], b[:, 3]) - np.maximum(boxes[i, 1], b[:, 1]))
        inter = w * h
        iou = inter / (area[i] + area[j] - inter)
        margins["iou"] = min(margins["iou"], float(np.abs(iou - thresh).min()))
        alive[j[(iou >= thresh) if mutant == "nms_greater_equal" else (iou > thresh)]] = False
    return kept


def proposals_one_image(heads, cell, strides, img_h, img_w, pre_topk, post_topk, nms_thresh, mutant=None) -> dict:
    """``heads``: five float32 arrays [H, W, head_ld] of ONE image (columns 0 .. 2 logits, 3 + 4 a + c deltas; columns from
    15 on are never looked at).  Returns boxes [post_topk, 4] f64 / scores [post_topk] f32 (zero beyond ``count``), ``src``
    [count, 4] = (level, h, w, a) and ``S`` [count, 2] of every output row, ``margins`` and ``dropped``."""
    thresh = float(np.float32(nms_thresh))
    margins = {"iou": math.inf, "extent": math.inf, "empty": math.inf}
    dropped = {"not_finite": 0, "empty": 0}
    rows = []                                                                   # per level: (boxes, scores, src, S) of the valid rows
    for lv, head in enumerate(heads):
        H, W = head.shape[0], head.shape[1]
        logits = np.ascontiguousarray(head[:, :, :3]).reshape(-1)
        sel = select(logits, pre_topk, mutant)
        aa, loc = sel % 3, sel // 3
        hh, ww = loc // W, loc % W
        deltas = head[hh, ww][:, 3:15].reshape(-1, 3, 4)[np.arange(sel.size), aa]
        scores = logits[sel]
        raw, S = decode(deltas, hh, ww, aa, cell[lv], int(strides[lv]), mutant)
        if mutant == "clip_before_finite_test":
            raw = clip(raw, img_h, img_w)
        finite = np.isfinite(raw).all(axis=1) & np.isfinite(scores)
        box = clip(raw, img_h, img_w)
        with np.errstate(all="ignore"):
            ew, eh = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
            nonempty = (ew > 0) & (eh > 0)
        valid = finite & nonempty
        dropped["not_finite"] += int((~finite).sum())
        dropped["empty"] += int((finite & ~nonempty).sum())
        # margins of the emptiness decisions (finite rows only)
        ext = np.concatenate([ew[valid], eh[valid]])
        if ext.size:
            margins["extent"] = min(margins["extent"], float(ext.min()))
        r = raw[finite & ~nonempty]
        if r.size:
            # a row that had a positive extent before clipping is empty BECAUSE of a clip plane: x2 <= 0, x1 >= img_w, ...;
            # its distance is the largest by which one of the planes is missed (one such axis is enough to empty the box)
            for lo, hi, size in ((r[:, 0], r[:, 2], float(img_w)), (r[:, 1], r[:, 3], float(img_h))):
                pos = hi - lo > 0
                out = pos & ((hi <= 0) | (lo >= size))
                if out.any():
                    dist = np.maximum(-hi[out], lo[out] - size)
                    margins["empty"] = min(margins["empty"], float(dist.min()))
        rows.append((box[valid], scores[valid], np.stack([np.full(sel.size, lv), hh, ww, aa], axis=1)[valid], S[valid]))
    boxes = np.concatenate([r[0] for r in rows])
    scores = np.concatenate([r[1] for r in rows])
    src = np.concatenate([r[2] for r in rows])
    S = np.concatenate([r[3] for r in rows])
    level = src[:, 0] if boxes.shape[0] else np.zeros(0, dtype=np.int64)
    if mutant == "nms_across_levels":
        # one greedy pass over all levels in merged order
        o = np.lexsort((np.arange(scores.size), -scores.astype(np.float64)))
        k = _greedy(boxes[o], np.zeros(o.size, dtype=np.int64), thresh, margins, mutant)
        kept = np.zeros(scores.size, dtype=bool)
        kept[o[k]] = True
    else:
        kept = _greedy(boxes, level, thresh, margins, mutant)                  # rows are in (level, rank) order already
    ki = np.nonzero(kept)[0]
    if mutant == "merge_by_level":
        order = ki
    else:
        order = ki[np.lexsort((ki, -scores[ki].astype(np.float64)))]           # ki ascending = (level, rank) ascending
    order = order[:post_topk]
    n = order.size
    out_b = np.zeros((post_topk, 4), dtype=np.float64)
    out_s = np.zeros((post_topk,), dtype=np.float32)
    out_b[:n], out_s[:n] = boxes[order], scores[order]
    return dict(boxes=out_b, scores=out_s, count=n, src=src[order], S=S[order], margins=margins, dropped=dropped,
                survivors=int(ki.size))


def proposals(heads, cell, strides, img_h, img_w, pre_topk, post_topk, nms_thresh, mutant=None) -> list:
    """``heads``: five arrays [N, H, W, head_ld]; one result of ``proposals_one_image`` per image."""
    n = heads[0].shape[0]
    return [proposals_one_image([h[i] for h in heads], cell, strides, img_h, img_w, pre_topk, post_topk, nms_thresh, mutant)
            for i in range(n)]


def all_candidates(heads, cell, strides, img_h, img_w) -> dict:
    """EVERY anchor of one image decoded and clipped: (level, h, w, a) [M, 4], score [M] f32, box [M, 4] f64 -- what an
    output row is matched against to recover where it came from."""
    src, score, box = [], [], []
    for lv, head in enumerate(heads):
        H, W = head.shape[0], head.shape[1]
        idx = np.arange(H * W * 3)
        aa, loc = idx % 3, idx // 3
        hh, ww = loc // W, loc % W
        deltas = head[:, :, 3:15].reshape(-1, 4)
        raw, _ = decode(deltas, hh, ww, aa, cell[lv], int(strides[lv]))
        box.append(clip(raw, img_h, img_w))
        score.append(np.ascontiguousarray(head[:, :, :3]).reshape(-1))
        src.append(np.stack([np.full(idx.size, lv), hh, ww, aa], axis=1))
    return dict(src=np.concatenate(src), score=np.concatenate(score), box=np.concatenate(box))
