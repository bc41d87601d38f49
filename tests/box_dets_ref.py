"""An independent reference for box detection selection (``demia_box_detections``): Detectron2 0.6
``FastRCNNOutputLayers.inference`` / ``fast_rcnn_inference_single_image`` with torchvision's hard NMS per class, restated
in plain numpy from the contract in ``include/deepemia_hip.h`` ("a3: Fast R-CNN inference").  No GPU, no import from the
project, and none of the kernel's structure: no packed keys, no sorting network, no chunks, no ballots -- one softmax, one
float64 decode, one ``lexsort``, one greedy loop.

Per image:
  * ROWS: the first ``min(prop_count, R)`` rows only; whatever lies behind them is never looked at.
  * SCORES: softmax over columns ``0 .. K`` in float64 from the float32 logits, the row maximum subtracted; column ``K`` is
    the background.  A row with any probability that is not finite is dropped (a ``+inf`` or NaN logit; a ``-inf`` logit
    gives a probability of 0 and the row stays).
  * DECODE in float64, class ``c`` from columns ``K + 1 + 4 c .. K + 4 + 4 c``: weights 10, 10, 5, 5; ``d / 5`` clamped at
    ``log(1000 / 16)`` with torch semantics (``np.minimum``: a NaN stays a NaN).  A row is dropped when a coordinate of ANY
    of its classes is not finite BEFORE clipping.  The contract is a float32 one, so "finite" means finite as a float32:
    not NaN and below ``F32_OVERFLOW`` in magnitude (a centre delta of 3e38 on a box 20 px wide is finite in float64 and is
    not a box).  Then clipped to ``[0, img_w] x [0, img_h]``.  NO emptiness filter: a box clipped to zero area stays.
  * CANDIDATES: the (row, class) pairs with ``score > thresh`` (strict), ordered by (score descending,
    ``row * K + class`` ascending).
  * NMS: greedy, per class, IoU in float64 with ``area = (x2 - x1)(y2 - y1)``, suppress when ``IoU > nms_thresh``; an IoU
    of 0 / 0 (two zero-area boxes) is NaN and suppresses nothing.  A suppressed box suppresses nothing.
  * OUTPUT: the first ``topk`` survivors.

Both thresholds are float32 numbers (they cross the C ABI as ``float``): the reference compares against their float32
values.

Besides the outputs every call returns how close its decisions were (``margins``) and why rows were dropped
(``dropped``).  ``margins``:
  ``score``   smallest |score - thresh| over every class of every row that was not dropped;
  ``gap``     smallest difference of two neighbouring candidates' scores (in candidate order) that are not bit-equal in the
              float32 restatement;
  ``iou``     smallest |IoU - nms_thresh| over the pairs the greedy pass tested;
  ``iou_rel`` smallest |IoU - nms_thresh| / |IoU_f32 - IoU| over those pairs, IoU_f32 the float32 quotient on boxes
              shifted by ``class * (max coordinate over the candidates + 1)`` and, likewise, on the plain float32 boxes;
  ``finite``  smallest distance of a finite-test decision: | log2 |v| - 128 | over every coordinate and every product
              the decode forms (binades from the float32 overflow threshold; NaN and infinite values decide themselves).
and the consistency counts ``tie_mismatch`` (neighbouring candidates that tie in one of float64 / float32 and not in the
other, or that tie although their logits are not bit-identical: such a tie hangs on the last bit of ``exp``) and ``iou_flips`` (tested pairs that float64, plain float32 and shifted float32 do not decide alike).
``tests/test_cpu_box_dets_ref.py`` holds the case table to minimum margins, so that no decision of the table can depend
on float32 against float64 rounding.

``dets_f32`` is the same computation in float32, one rounding per operation, no FMA, in the order a float32
implementation of Detectron2's ``apply_deltas`` takes; with at most 1000 candidates its NMS quotient is taken on the
shifted boxes (torchvision's ``batched_nms`` below 4000 coordinates), above that on the plain ones.  It MEASURES what
float32 costs; it is not a second reference.

``mutant`` switches ONE deliberate mistake on (the CPU test shows that the case table notices each of them).
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64

SCALE_CLAMP = math.log(1000.0 / 16)
WEIGHTS = (10.0, 10.0, 5.0, 5.0)
F32_OVERFLOW = (2.0 - 2.0 ** -24) * 2.0 ** 127          # from here on a number rounds to infinity in float32
MUTANTS = ("background_first", "threshold_greater_equal", "nms_greater_equal", "nms_across_classes", "suppressed_still_suppress",
           "drop_class_not_row", "clip_before_finite_test", "no_clamp", "clamp_before_weight", "weights_swapped",
           "drop_empty_boxes", "tie_order_reversed", "topk_before_nms", "rows_past_count_used")


def softmax(logits: np.ndarray, dt) -> np.ndarray:
    """Row softmax of ``logits`` [R, K + 1] (float32) in ``dt``: maximum subtracted, the sum taken column after column."""
    x = logits.astype(dt)
    with np.errstate(all="ignore"):
        e = np.exp(x - x.max(axis=1, keepdims=True))
        s = e[:, 0].copy()
        for c in range(1, x.shape[1]):
            s = s + e[:, c]
        p = e / s[:, None]
    assert p.dtype == dt
    return p


def decode(deltas: np.ndarray, props: np.ndarray, dt, mutant=None):
    """Boxes [R, K, 4] BEFORE clipping of ``props`` [R, 4] with their ``deltas`` [R, K, 4] in ``dt``, the scale ``S``
    [R, K, 2] (x, y) of the arithmetic (|centre| + |d size| + exp(dsize) size bounds every intermediate), and every value
    the finite test can hang on [R, K, 8]: the four coordinates and the four products behind them."""
    p = props.astype(dt)
    d = deltas.astype(dt)
    wx, wy, ww, wh = (dt(w) for w in WEIGHTS)
    if mutant == "weights_swapped":
        wx, wy, ww, wh = ww, wh, wx, wy
    half, clamp = dt(0.5), dt(SCALE_CLAMP)
    with np.errstate(all="ignore"):
        wd, ht = (p[:, 2] - p[:, 0])[:, None], (p[:, 3] - p[:, 1])[:, None]
        cx, cy = p[:, 0][:, None] + half * wd, p[:, 1][:, None] + half * ht
        dx, dy = d[..., 0] / wx, d[..., 1] / wy
        if mutant == "clamp_before_weight":
            dw, dh = np.minimum(d[..., 2], clamp) / ww, np.minimum(d[..., 3], clamp) / wh
        elif mutant == "no_clamp":
            dw, dh = d[..., 2] / ww, d[..., 3] / wh
        else:
            dw, dh = np.minimum(d[..., 2] / ww, clamp), np.minimum(d[..., 3] / wh, clamp)     # np.minimum keeps a NaN, as torch.clamp does
        sx, sy = dx * wd, dy * ht
        pcx, pcy = sx + cx, sy + cy
        pw, ph = np.exp(dw) * wd, np.exp(dh) * ht
        box = np.stack([pcx - half * pw, pcy - half * ph, pcx + half * pw, pcy + half * ph], axis=-1)
        S = np.stack([np.abs(cx) + np.abs(sx) + pw, np.abs(cy) + np.abs(sy) + ph], axis=-1)
        parts = np.concatenate([box, np.stack([sx, sy, pw, ph], axis=-1)], axis=-1)
    assert box.dtype == dt
    return box, S, parts


def clip(box: np.ndarray, img_h: int, img_w: int) -> np.ndarray:
    out = box.copy()
    with np.errstate(all="ignore"):
        out[..., 0::2] = np.clip(box[..., 0::2], box.dtype.type(0), box.dtype.type(img_w))
        out[..., 1::2] = np.clip(box[..., 1::2], box.dtype.type(0), box.dtype.type(img_h))
    return out


def finite_as_f32(v: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        return np.isfinite(v) & (np.abs(v) < F32_OVERFLOW)


def iou_of(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """IoU of box ``a`` [4] with boxes ``b`` [m, 4] in their own dtype, one rounding per operation; 0 / 0 is NaN."""
    zero = a.dtype.type(0)
    with np.errstate(all="ignore"):
        aa = (a[2] - a[0]) * (a[3] - a[1])
        ab = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        w = np.maximum(zero, np.minimum(a[2], b[:, 2]) - np.maximum(a[0], b[:, 0]))
        h = np.maximum(zero, np.minimum(a[3], b[:, 3]) - np.maximum(a[1], b[:, 1]))
        inter = w * h
        out = inter / (aa + ab - inter)
    assert out.dtype == a.dtype
    return out


def shifted_f32(boxes32: np.ndarray, cls: np.ndarray) -> np.ndarray:
    """torchvision's coordinate trick in float32: every box moved by ``class * (boxes.max() + 1)``."""
    if boxes32.shape[0] == 0:
        return boxes32
    step = boxes32.max() + f32(1)
    out = boxes32 + (cls.astype(f32) * step)[:, None]
    assert out.dtype == f32
    return out


def greedy(boxes: np.ndarray, group: np.ndarray, thresh, mutant=None, margins=None, also=()) -> np.ndarray:
    """Greedy hard NMS of ``boxes`` [m, 4] in the given order; rows of different ``group`` never meet.  Returns the kept mask.
    With ``margins``, every tested pair's distance from the threshold is booked, and its float32 quotients on each box set
    of ``also`` are compared with it."""
    m = boxes.shape[0]
    alive = np.ones(m, dtype=bool)
    kept = np.zeros(m, dtype=bool)
    for i in range(m):
        if not alive[i]:
            if mutant != "suppressed_still_suppress":
                continue
        else:
            kept[i] = True
        j = np.nonzero(alive[i + 1:] & (group[i + 1:] == group[i]))[0] + i + 1
        if j.size == 0:
            continue
        iou = iou_of(boxes[i], boxes[j])
        with np.errstate(all="ignore"):
            hit = (iou >= thresh) if mutant == "nms_greater_equal" else (iou > thresh)
        if margins is not None:
            ok = ~np.isnan(iou)
            dist = np.abs(iou - float(thresh))
            if ok.any():
                margins["iou"] = min(margins["iou"], float(dist[ok].min()))
            for b32 in also:
                q = iou_of(b32[i], b32[j])
                margins["iou_flips"] += int(((q > f32(thresh)) != hit).sum()) + int((np.isnan(q) != np.isnan(iou)).sum())
                err = np.abs(q.astype(f64) - iou)
                with np.errstate(all="ignore"):
                    rel = np.where(err > 0, dist / err, np.inf)
                if ok.any():
                    margins["iou_rel"] = min(margins["iou_rel"], float(rel[ok].min()))
        alive[j[hit]] = False
    return kept


def _prepare(logits, props, prop_count, K, dt, mutant):
    R = logits.shape[0]
    rows = R if mutant == "rows_past_count_used" else max(0, min(int(prop_count), R))
    lg, pr = logits[:rows], props[:rows]
    p = softmax(lg[:, :K + 1], dt)
    scores = p[:, 1:K + 1] if mutant == "background_first" else p[:, :K]
    deltas = lg[:, K + 1:K + 1 + 4 * K].reshape(rows, K, 4)
    raw, S, parts = decode(deltas, pr, dt, mutant)
    return rows, p, scores, raw, S, parts


def detections_one_image(logits, props, prop_count, K, img_h, img_w, score_thresh, nms_thresh, topk, mutant=None) -> dict:
    """``logits`` [R, ld] float32 (columns ``0 .. K`` class logits, ``K + 1 .. 5 K`` deltas; columns from ``5 K + 1`` on are
    never looked at), ``props`` [R, 4] float32 of ONE image.  Returns boxes [topk, 4] f64, scores [topk] f64, classes
    [topk] (zero beyond ``count``), ``src`` [count, 2] = (row, class), ``S`` [count, 2] and ``rank`` [count] (the place in
    candidate order) of every output row, the number
    of candidates and of survivors before the cut, ``margins`` and ``dropped`` ({row: reason})."""
    s_thr, n_thr = float(f32(score_thresh)), float(f32(nms_thresh))
    rows, p, scores, raw, S, parts = _prepare(logits, props, prop_count, K, f64, mutant)
    _, p32, scores32, raw32, _, _ = _prepare(logits, props, prop_count, K, f32, mutant)
    margins = {"score": math.inf, "gap": math.inf, "iou": math.inf, "iou_rel": math.inf, "finite": math.inf, "tie_mismatch": 0, "iou_flips": 0}
    # ---- which rows are dropped, and why
    bad_score = ~np.isfinite(p).all(axis=1)
    tested = clip(raw, img_h, img_w) if mutant == "clip_before_finite_test" else raw
    fin = finite_as_f32(tested)                                                  # [rows, K, 4]
    if mutant == "drop_class_not_row":
        bad_box_rc = ~fin.all(axis=2)                                            # [rows, K]
        bad_box = np.zeros(rows, dtype=bool)
    else:
        bad_box = ~fin.all(axis=(1, 2))
        bad_box_rc = np.zeros((rows, K), dtype=bool)
    dropped = {int(r): ("score_not_finite" if bad_score[r] else "box_not_finite") for r in np.nonzero(bad_score | bad_box)[0]}
    live = ~(bad_score | bad_box)
    with np.errstate(all="ignore"):
        v = np.abs(parts[live])
        v = v[np.isfinite(v) & (v > 0)]
    if v.size:
        margins["finite"] = float(np.abs(np.log2(v) - 128.0).min())
    box = clip(raw, img_h, img_w)
    box32 = clip(raw32, img_h, img_w)
    # ---- candidates
    with np.errstate(all="ignore"):
        cand = (scores >= s_thr) if mutant == "threshold_greater_equal" else (scores > s_thr)
    cand &= live[:, None] & ~bad_box_rc
    if mutant == "drop_empty_boxes":
        cand &= (box[..., 2] - box[..., 0] > 0) & (box[..., 3] - box[..., 1] > 0)
    if live.any():
        margins["score"] = float(np.abs(scores[live] - s_thr).min())
    rr, cc = np.nonzero(cand)
    ident = rr * K + cc
    sc = scores[rr, cc]
    order = np.lexsort((-ident if mutant == "tie_order_reversed" else ident, -sc))
    rr, cc, sc = rr[order], cc[order], sc[order]
    sc32 = scores32[rr, cc]
    if sc.size > 1:
        same32 = sc32[:-1].view(np.uint32) == sc32[1:].view(np.uint32)
        same64 = sc[:-1] == sc[1:]
        # a tie is founded when the two rows' class logits are bit-identical and so are the two classes' logits: then every
        # implementation computes the same number twice, whatever its exp
        cl = logits[:, :K + 1].view(np.uint32)
        founded = (cl[rr[:-1]] == cl[rr[1:]]).all(axis=1) & (cl[rr[:-1], cc[:-1]] == cl[rr[1:], cc[1:]])
        margins["tie_mismatch"] = int((same32 != same64).sum()) + int((same64 & ~founded).sum())
        gaps = (sc[:-1] - sc[1:])[~same32]
        if gaps.size:
            margins["gap"] = float(gaps.min())
    ncand = int(sc.size)
    if mutant == "topk_before_nms":
        rr, cc, sc = rr[:topk], cc[:topk], sc[:topk]
    # ---- NMS
    cb, cb32 = box[rr, cc], box32[rr, cc]
    group = np.zeros_like(cc) if mutant == "nms_across_classes" else cc
    kept = greedy(cb, group, n_thr, mutant, margins, also=(cb32, shifted_f32(cb32, cc)))
    ki = np.nonzero(kept)[0]
    out = ki[:topk]
    n = int(out.size)
    out_b, out_s, out_c = np.zeros((topk, 4), dtype=f64), np.zeros((topk,), dtype=f64), np.zeros((topk,), dtype=np.int64)
    out_b[:n], out_s[:n], out_c[:n] = cb[out], sc[out], cc[out]
    return dict(boxes=out_b, scores=out_s, classes=out_c, count=n, src=np.stack([rr[out], cc[out]], axis=1), S=S[rr[out], cc[out]], rank=out,
                ncand=ncand, survivors=int(ki.size), margins=margins, dropped=dropped,
                max_coord_holders=(int((cb.max(axis=1) == cb.max()).sum()) if ncand else 0),
                max_coord_src=((int(rr[int(cb.max(axis=1).argmax())]), int(cc[int(cb.max(axis=1).argmax())])) if ncand else None))


def detections(logits, props, prop_count, K, img_h, img_w, score_thresh, nms_thresh, topk, mutant=None) -> list:
    """``logits`` [N, R, ld], ``props`` [N, R, 4], ``prop_count`` [N]; one result of ``detections_one_image`` per image."""
    return [detections_one_image(logits[n], props[n], int(prop_count[n]), K, img_h, img_w, score_thresh, nms_thresh, topk, mutant)
            for n in range(logits.shape[0])]


def dets_f32(logits, props, prop_count, K, img_h, img_w, score_thresh, nms_thresh, topk) -> dict:
    """One image in float32 throughout: boxes [count, 4] and scores [count] float32, classes, ``src`` and ``count``."""
    rows, p, scores, raw, _, _ = _prepare(logits, props, prop_count, K, f32, None)
    live = np.isfinite(p).all(axis=1) & np.isfinite(raw).all(axis=(1, 2))
    box = clip(raw, img_h, img_w)
    with np.errstate(all="ignore"):
        cand = (scores > f32(score_thresh)) & live[:, None]
    rr, cc = np.nonzero(cand)
    sc = scores[rr, cc]
    order = np.lexsort((rr * K + cc, -sc.astype(f64)))
    rr, cc, sc = rr[order], cc[order], sc[order]
    cb = box[rr, cc]
    nms_boxes = shifted_f32(cb, cc) if 4 * sc.size <= 4000 else cb
    out = np.nonzero(greedy(nms_boxes, cc, f32(nms_thresh)))[0][:topk]
    assert cb.dtype == f32 and sc.dtype == f32
    return dict(boxes=cb[out], scores=sc[out], classes=cc[out], src=np.stack([rr[out], cc[out]], axis=1), count=int(out.size))
