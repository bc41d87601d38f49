"""Plain-Python restatements of the pycocotools pieces the evaluate task relies on -- the checkers of the evaluate tests.

``fr_poly`` (maskApi.c ``rleFrPoly``), ``encode`` / ``decode`` (column-major runs, background first), ``to_string``
(``rleToString``), ``coco_eval`` (``COCOeval`` with ``useCats=1``: ``evaluate`` / ``accumulate`` / ``summarize`` written
loop by loop as pycocotools writes them) and Detectron2's ``convert_to_coco_dict`` for the custom label JSON.  Neither
pycocotools nor Detectron2 is available to pin these against; they are written from the algorithms' published source.
"""
import json
import math
import os

import numpy as np

INT_MIN = -2 ** 31


def fr_poly(xy, h, w):
    """rleFrPoly: run lengths of one polygon (flat x, y list) in an h x w frame."""
    k = len(xy) // 2
    x = [int(5 * xy[2 * j] + .5) for j in range(k)]
    y = [int(5 * xy[2 * j + 1] + .5) for j in range(k)]
    x.append(x[0] if k else 0)
    y.append(y[0] if k else 0)
    u, v = [], []
    for j in range(k):
        xs, xe, ys, ye = x[j], x[j + 1], y[j], y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        if dx >= dy:
            s = (ye - ys) / dx if dx else float("nan")      # 0 / 0 in C: NaN, and (int)NaN is INT_MIN on x86
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                val = ys + s * t + .5
                v.append(INT_MIN if val != val else int(val))
        else:
            s = (xe - xs) / dy
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                u.append(int(xs + s * t + .5))
    pts = []
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
        xd = (xd + .5) / 5 - .5
        if math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
        yd = (yd + .5) / 5 - .5
        yd = 0.0 if yd < 0 else (float(h) if yd > h else yd)
        pts.append(int(xd) * h + int(math.ceil(yd)))
    a = sorted(pts + [h * w])
    p, d = 0, []
    for t in a:
        d.append(t - p)
        p = t
    b, j = [d[0]], 1
    while j < len(d):
        if d[j] > 0:
            b.append(d[j])
            j += 1
        else:
            j += 1
            if j < len(d):
                b[-1] += d[j]
                j += 1
    return b


def decode(counts, h, w):
    flat = np.zeros(h * w, dtype=bool)
    pos = 0
    for i, c in enumerate(counts):
        if i % 2:
            flat[pos:pos + c] = True
        pos += c
    return flat.reshape(w, h).T


def poly_mask(polys, h, w):
    """frPyObjects + merge: the union of the polygons' masks."""
    m = np.zeros((h, w), dtype=bool)
    for p in polys:
        m |= decode(fr_poly(list(p), h, w), h, w)
    return m


def encode(mask):
    flat = np.asarray(mask, dtype=bool).T.reshape(-1)
    counts, p, c = [], False, 0
    for b in flat:
        if b != p:
            counts.append(c)
            c = 0
            p = b
        c += 1
    counts.append(c)
    return counts


def to_string(counts):
    out = []
    for i, c in enumerate(counts):
        x = int(c)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            ch = x & 0x1f
            x >>= 5
            more = (x != -1) if (ch & 0x10) else (x != 0)
            if more:
                ch |= 0x20
            out.append(chr(ch + 48))
    return "".join(out)


def from_string(s):
    cnts, p = [], 0
    while p < len(s):
        x = k = 0
        more = True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return cnts


def split_rule(files, test_size=0.2, seed=42):
    n = len(files)
    n_test = int(math.ceil(test_size * n))
    perm = np.random.RandomState(seed).permutation(n)
    return [files[i] for i in perm[n_test:]], [files[i] for i in perm[:n_test]]


def gt_from_label_files(label_dir, files, classes, ellipse_polygon):
    """convert_to_coco_dict of the reference's get_split_dicts records: (images, annotations) with ids from 1."""
    images, anns = [], []
    for idx, fn in enumerate(files):
        lab = json.load(open(os.path.join(label_dir, fn)))
        md = lab["metadata"]
        images.append({"id": idx, "height": md["height"], "width": md["width"]})
        for inst in lab["instances"]:
            if inst["className"] not in classes:
                continue
            if inst["type"] == "polygon":
                pts = inst["points"]
                px, py = list(pts[0:-1:2]) + [pts[0]], list(pts[1:-1:2]) + [pts[-1]]
            else:
                px, py = ellipse_polygon(inst["cx"], inst["cy"], inst["rx"], inst["ry"], inst["angle"])
                px, py = list(px), list(py)
            poly = [c for x, y in zip(px, py) for c in (x + 0.5, y + 0.5)]
            xs, ys = np.array(poly[0::2]), np.array(poly[1::2])
            area = float(np.float32(0.5 * abs(np.dot(xs, np.roll(ys, 1)) - np.dot(ys, np.roll(xs, 1)))))
            x0, y0, x1, y1 = float(np.min(px)), float(np.min(py)), float(np.max(px)), float(np.max(py))
            anns.append({"id": len(anns) + 1, "image_id": idx, "category_id": classes.index(inst["className"]), "iscrowd": 0,
                         "segmentation": [poly], "area": area,
                         "bbox": [round(v, 3) for v in (x0, y0, x1 - x0, y1 - y0)]})
    return images, anns


def coco_eval(images, gts, dts, cat_ids, iou_type, iou_lookup=None, dt_area=None):
    """COCOeval(useCats=1).evaluate() / accumulate() / summarize(): (stats [12], precision [T, R, K, A, M]).
    ``iou_lookup(d, g)`` / ``dt_area(d)`` (optional) replace the IoU and the detection area computed from the masks / boxes."""
    iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
    rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
    max_dets = [1, 10, 100]
    area_rng = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]
    img_ids = sorted(im["id"] for im in images)
    hw = {im["id"]: (im["height"], im["width"]) for im in images}
    dts = [dict(d, id=i + 1, iscrowd=0) for i, d in enumerate(dts)]
    for d in dts:
        if dt_area is not None:
            d["area"] = dt_area(d)
        elif iou_type == "bbox":
            d["area"] = d["bbox"][2] * d["bbox"][3]
        else:
            d["area"] = float(sum(from_string(d["segmentation"]["counts"])[1::2]))
    mask_cache = {}

    def mask_of(o, kind):
        key = (kind, o["id"])
        if key not in mask_cache:
            h, w = hw[o["image_id"]]
            if kind == "gt":
                mask_cache[key] = poly_mask(o["segmentation"], h, w)
            else:
                mask_cache[key] = decode(from_string(o["segmentation"]["counts"]), h, w)
        return mask_cache[key]

    _g, _d = {}, {}
    for g in gts:
        g = dict(g, ignore=int(g.get("iscrowd", 0)))
        _g.setdefault((g["image_id"], g["category_id"]), []).append(g)
    for d in dts:
        _d.setdefault((d["image_id"], d["category_id"]), []).append(d)

    def compute_iou(i, c):
        gt, dt = _g.get((i, c), []), _d.get((i, c), [])
        if not gt and not dt:
            return []
        inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[j] for j in inds][:max_dets[-1]]
        if not gt or not dt:
            return []
        out = np.zeros((len(dt), len(gt)))
        for a, d in enumerate(dt):
            for b, g in enumerate(gt):
                crowd = g.get("iscrowd", 0)
                if iou_lookup is not None:
                    out[a, b] = iou_lookup(d, g)
                    continue
                if iou_type == "bbox":
                    D, G = d["bbox"], g["bbox"]
                    ww = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
                    hh = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
                    if ww <= 0 or hh <= 0:
                        continue
                    inter = ww * hh
                    u = D[2] * D[3] if crowd else D[2] * D[3] + G[2] * G[3] - inter
                else:
                    md, mg = mask_of(d, "dt"), mask_of(g, "gt")
                    inter = float(np.count_nonzero(md & mg))
                    if inter == 0:
                        continue
                    u = float(md.sum()) if crowd else float(md.sum() + mg.sum()) - inter
                out[a, b] = inter / u
        return out

    ious = {(i, c): compute_iou(i, c) for i in img_ids for c in cat_ids}

    def evaluate_img(i, c, rng, max_det):
        gt, dt = _g.get((i, c), []), _d.get((i, c), [])
        if not gt and not dt:
            return None
        for g in gt:
            g["_ignore"] = 1 if (g["ignore"] or g["area"] < rng[0] or g["area"] > rng[1]) else 0
        gtind = np.argsort([g["_ignore"] for g in gt], kind="mergesort")
        gt = [gt[j] for j in gtind]
        dtind = np.argsort([-d["score"] for d in dt], kind="mergesort")
        dt = [dt[j] for j in dtind[0:max_det]]
        iscrowd = [int(o.get("iscrowd", 0)) for o in gt]
        tab = ious[i, c][:, gtind] if len(ious[i, c]) > 0 else ious[i, c]
        T, G, D = len(iou_thrs), len(gt), len(dt)
        gtm, dtm = np.zeros((T, G)), np.zeros((T, D))
        gt_ig = np.array([g["_ignore"] for g in gt])
        dt_ig = np.zeros((T, D))
        if len(tab):
            for ti, t in enumerate(iou_thrs):
                for di, d in enumerate(dt):
                    iou = min([t, 1 - 1e-10])
                    m = -1
                    for gi, g in enumerate(gt):
                        if gtm[ti, gi] > 0 and not iscrowd[gi]:
                            continue
                        if m > -1 and gt_ig[m] == 0 and gt_ig[gi] == 1:
                            break
                        if tab[di, gi] < iou:
                            continue
                        iou = tab[di, gi]
                        m = gi
                    if m == -1:
                        continue
                    dt_ig[ti, di] = gt_ig[m]
                    dtm[ti, di] = gt[m]["id"]
                    gtm[ti, m] = d["id"]
        a = np.array([d["area"] < rng[0] or d["area"] > rng[1] for d in dt]).reshape((1, len(dt)))
        dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
        return {"dtMatches": dtm, "dtScores": [d["score"] for d in dt], "gtIgnore": gt_ig, "dtIgnore": dt_ig}

    evals = [evaluate_img(i, c, r, max_dets[-1]) for c in cat_ids for r in area_rng for i in img_ids]
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), len(cat_ids), len(area_rng), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    I0, A0 = len(img_ids), len(area_rng)
    for k in range(K):
        for a in range(A):
            for mi, md in enumerate(max_dets):
                E = [evals[k * A0 * I0 + a * I0 + i] for i in range(I0)]
                E = [e for e in E if e is not None]
                if not E:
                    continue
                sc = np.concatenate([np.asarray(e["dtScores"][0:md], dtype=np.float64) for e in E])
                inds = np.argsort(-sc, kind="mergesort")
                dtm = np.concatenate([e["dtMatches"][:, 0:md] for e in E], axis=1)[:, inds]
                dtig = np.concatenate([e["dtIgnore"][:, 0:md] for e in E], axis=1)[:, inds]
                gtig = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gtig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dtig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dtig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, mi] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    ids = np.searchsorted(rc, rec_thrs, side="left")
                    try:
                        for ri, pi in enumerate(ids):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, mi] = np.array(q)

    def summ(ap=1, thr=None, area="all", md=100):
        aind = ["all", "small", "medium", "large"].index(area)
        mind = max_dets.index(md)
        if ap == 1:
            s = precision
            if thr is not None:
                s = s[np.where(thr == iou_thrs)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = recall
            if thr is not None:
                s = s[np.where(thr == iou_thrs)[0]]
            s = s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])

    stats = np.array([summ(1), summ(1, .5), summ(1, .75), summ(1, area="small"), summ(1, area="medium"), summ(1, area="large"),
                      summ(0, md=1), summ(0, md=10), summ(0), summ(0, area="small"), summ(0, area="medium"), summ(0, area="large")])
    return stats, precision


def derive(stats, precision, names):
    metrics = ["AP", "AP50", "AP75", "APs", "APm", "APl"]
    res = {m: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, m in enumerate(metrics)}
    for k, n in enumerate(names):
        p = precision[:, :, k, 0, -1]
        p = p[p > -1]
        res["AP-" + n] = float((np.mean(p) if p.size else float("nan")) * 100)
    return res
