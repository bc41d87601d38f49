"""Dense NumPy reference of the outline-agreement stage (``demia_mask_outline_agreement``; the definitions are stated in
``include/deepemia_hip.h``): the border by four shifts, ``d2`` by int64 broadcasting over the two point sets, ``q`` by
``math.isqrt``, the bins by a search over integers -- and the report's seven values as f64 formulas on those integers.  Nothing
here shares code with the library."""
import math

import numpy as np

BINS = 128


def border(mask: np.ndarray) -> np.ndarray:
    """The set pixels with an unset 4-neighbour; outside the frame counts as unset."""
    m = np.asarray(mask, dtype=bool)
    p = np.pad(m, 1)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return m & ~inner


def points(mask: np.ndarray) -> np.ndarray:
    """``[n, 2]`` int64 (y, x) of the border pixels."""
    ys, xs = np.nonzero(border(mask))
    return np.stack([ys, xs], 1).astype(np.int64)


def min_d2(src_pts: np.ndarray, tgt_pts: np.ndarray, rows: int = 256) -> np.ndarray:
    """For every source point the minimum squared distance to the target points, int64, by broadcasting (``rows`` at a time)."""
    out = np.zeros(len(src_pts), dtype=np.int64)
    for i in range(0, len(src_pts), rows):
        d = src_pts[i:i + rows, None, :] - tgt_pts[None, :, :]
        out[i:i + rows] = (d * d).sum(-1).min(1)
    return out


def q(d2: int) -> int:
    return math.isqrt(int(d2) << 16)


def bin_of(d2: int) -> int:
    c = 0
    while c * c < d2 and c < BINS - 1:
        c += 1
    return c


def directed(src: np.ndarray, tgt: np.ndarray) -> dict:
    """One record: source ``src`` against target ``tgt`` (dense masks)."""
    sp, tp = points(src), points(tgt)
    rec = {"n": len(sp), "max_d2": 0, "sum_d2": 0, "sum_q": 0, "hist": [0] * BINS}
    if len(sp) == 0 or len(tp) == 0:
        return rec
    d2 = min_d2(sp, tp).tolist()
    rec["max_d2"], rec["sum_d2"], rec["sum_q"] = max(d2), sum(d2), sum(q(v) for v in d2)
    for v in d2:
        rec["hist"][bin_of(v)] += 1
    return rec


def records(det: np.ndarray, gt: np.ndarray, pairs) -> dict:
    """What ``OutlineAgreement.from_host`` returns, for dense ``det`` [D, H, W], ``gt`` [G, H, W] and ``pairs`` [P, 2]."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    P = len(pairs)
    out = {k: np.zeros((P, 2), dtype=np.int64) for k in ("n", "max_d2", "sum_d2", "sum_q")}
    out["hist"] = np.zeros((P, 2, BINS), dtype=np.int64)
    cache = {}
    for p, (d, g) in enumerate(pairs.tolist()):
        for direction, key in enumerate(((0, d, g), (1, d, g))):
            if key not in cache:
                cache[key] = directed(det[d], gt[g]) if direction == 0 else directed(gt[g], det[d])
            r = cache[key]
            for k in ("n", "max_d2", "sum_d2", "sum_q"):
                out[k][p, direction] = r[k]
            out["hist"][p, direction] = r["hist"]
    return out


def values(dg: dict, gd: dict, a_d: int, a_g: int, tolerance: int) -> dict:
    """The report's seven values of one pair from its two records (``dg``: detection -> annotation, ``gd``: the reverse) and the
    two pixel counts: f64 formulas applied to integers."""
    n_d, n_g = int(dg["n"]), int(gd["n"])
    cum_dg, cum_gd = np.cumsum(dg["hist"]).tolist(), np.cumsum(gd["hist"]).tolist()

    def hd95(cum, n):
        return next(c for c in range(BINS) if 100 * cum[c] >= 95 * n)
    return {"assd": (int(dg["sum_q"]) + int(gd["sum_q"])) / (256 * (n_d + n_g)),
            "rms": math.sqrt((int(dg["sum_d2"]) + int(gd["sum_d2"])) / (n_d + n_g)),
            "hausdorff": math.sqrt(max(int(dg["max_d2"]), int(gd["max_d2"]))),
            "hd95": float(max(hd95(cum_dg, n_d), hd95(cum_gd, n_g))),
            "nsd": (cum_dg[tolerance] + cum_gd[tolerance]) / (n_d + n_g),
            "diameter_error": 2 * math.sqrt(a_d / math.pi) - 2 * math.sqrt(a_g / math.pi),
            "area_error": (a_d - a_g) / a_g}


def match(iou: np.ndarray, scores, d_cat, g_cat, crowd, thr: float):
    """The matching rule, brute force: detections in descending score (ties: ascending index); each takes, among the annotations
    that are still free, not crowd, of its category and with IoU >= ``thr``, the one of the highest IoU (ties: the lower index).
    ``[(detection, annotation)]`` sorted by detection."""
    D, G = len(scores), len(g_cat)
    order = sorted(range(D), key=lambda i: (-float(scores[i]), i))
    taken, out = set(), []
    for d in order:
        best = None
        for g in range(G):
            if g in taken or int(crowd[g]) or int(g_cat[g]) != int(d_cat[d]) or not float(iou[d, g]) >= thr:
                continue
            if best is None or float(iou[d, g]) > float(iou[d, best]):
                best = g
        if best is not None:
            taken.add(best)
            out.append((d, best))
    return sorted(out)
