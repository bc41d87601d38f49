"""Extensions of ``coco_ref`` for the pipeline mode of the evaluate task, written the same way (plain restatements of
pycocotools' published source; ``coco_ref.py`` itself stays as it is):

``coco_eval``   ``coco_ref.coco_eval`` with ``params.maxDets`` as an argument.  The function is ``coco_ref``'s own text with its
                three literals of maxDets replaced (the list, ``summarize``'s default and the two small AR entries), so the
                matching and accumulation are the very loops the existing tests check.
``to_bbox``     ``rleToBbox`` (pycocotools 2.0.7 on), run by run.
``encode``      ``coco_ref.encode`` with numpy instead of a loop over pixels (for 2048^2 frames).
``encode_pixels`` / ``runs_to_pixels``  the same run lengths from / to the sorted column-major positions of the set pixels.
``cross_counts``  ``|det_i & gt_j|`` of sets of small masks from their pixel lists (no [D, G, H, W] array).
"""
import inspect

import numpy as np

import coco_ref as R

_EDITS = [("    max_dets = [1, 10, 100]\n", "    max_dets = list(MAX_DETS)\n"),
          ('    def summ(ap=1, thr=None, area="all", md=100):\n', '    def summ(ap=1, thr=None, area="all", md=None):\n'),
          ("        mind = max_dets.index(md)\n", "        mind = max_dets.index(max_dets[-1] if md is None else md)\n"),
          ("summ(0, md=1), summ(0, md=10), summ(0),", "summ(0, md=max_dets[0]), summ(0, md=max_dets[1]), summ(0),")]


def coco_eval(images, gts, dts, cat_ids, iou_type, max_dets, iou_lookup=None, dt_area=None):
    """``coco_ref.coco_eval`` at ``params.maxDets = max_dets``: every AP and the area ARs at its last entry."""
    src = inspect.getsource(R.coco_eval)
    for old, new in _EDITS:
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    ns = dict(vars(R), MAX_DETS=list(max_dets))
    exec(compile(src, "coco_ref.coco_eval[max_dets]", "exec"), ns)
    return ns["coco_eval"](images, gts, dts, cat_ids, iou_type, iou_lookup=iou_lookup, dt_area=dt_area)


def to_bbox(counts, h, w):
    """rleToBbox of one run list (background first, column-major): [x, y, w, h] floats."""
    m = (len(counts) // 2) * 2
    if m == 0:
        return [0.0, 0.0, 0.0, 0.0]
    xs, ys, xe, ye, cc = w, h, 0, 0, 0
    for j in range(m):
        start = cc
        cc += int(counts[j])
        if j % 2 == 0 or int(counts[j]) == 0:
            continue
        y_start = start % h
        x_start = (start - y_start) // h
        y_end = (cc - 1) % h
        x_end = (cc - 1 - y_end) // h
        xs, xe = min(xs, x_start), max(xe, x_end)
        if x_start < x_end:
            ys, ye = 0, h - 1                       # the run goes on into the next column
        else:
            ys, ye = min(ys, y_start), max(ye, y_end)
    return [float(xs), float(ys), float(xe - xs + 1), float(ye - ys + 1)]


def encode(mask):
    """``coco_ref.encode`` (column-major run lengths, the background run first) without the pixel loop."""
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)
    edges = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    pos = np.concatenate([[0], edges, [flat.size]])
    counts = np.diff(pos).tolist()
    return ([0] + counts) if flat.size and flat[0] else counts


def encode_pixels(pos, total):
    """Run lengths of the mask whose set pixels sit at the sorted column-major positions ``pos`` of a ``total``-pixel frame."""
    pos = np.asarray(pos, dtype=np.int64)
    if pos.size == 0:
        return [int(total)]
    brk = np.flatnonzero(np.diff(pos) != 1)
    starts = np.concatenate([[pos[0]], pos[brk + 1]])
    ends = np.concatenate([pos[brk], [pos[-1]]]) + 1
    edges = np.stack([starts, ends], 1).reshape(-1)
    counts = np.diff(np.concatenate([[0], edges])).tolist()
    if ends[-1] != total:
        counts.append(int(total - ends[-1]))
    return counts


def runs_to_pixels(counts):
    """Sorted column-major positions of the set pixels of a run list (background first)."""
    c = np.asarray(counts, dtype=np.int64)
    end = np.cumsum(c)
    fg = np.arange(len(c)) % 2 == 1
    n = c[fg]
    if n.sum() == 0:
        return np.zeros(0, dtype=np.int64)
    start = (end - c)[fg]
    return np.repeat(start, n) + (np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n))


def cross_counts(det_pix, gt_pix, D, G):
    """``[D, G]`` int64 intersection counts; ``det_pix`` / ``gt_pix`` = (mask index, flat pixel index) arrays of the set pixels."""
    di, dp = det_pix
    gi, gp = gt_pix
    order = np.argsort(dp, kind="mergesort")
    di, dp = di[order], dp[order]
    lo, hi = np.searchsorted(dp, gp, side="left"), np.searchsorted(dp, gp, side="right")
    n = hi - lo
    rows = di[np.repeat(lo, n) + (np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n))]
    cols = np.repeat(gi, n)
    out = np.zeros((D, G), dtype=np.int64)
    np.add.at(out, (rows, cols), 1)
    return out
