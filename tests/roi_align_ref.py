"""An independent reference for the ROI pooler: torchvision 0.11 ``roi_align`` (aligned=True, sampling_ratio=0) and
detectron2's ``assign_boxes_to_levels``, restated in plain numpy.  No GPU, no import from the project.

The DIRECT form on purpose: loop over bins, loop over samples, four taps per sample -- no separable weight tables, no row
cache, no pairing of bin columns, so that it shares no structure with ``csrc/roialign.hip``.

Two number formats, for a reason:
  * the GEOMETRY is float32 in torchvision's operation order (scale, the -0.5 offset, bin size, ``ceil``, the sample
    coordinate ``start + b * bsz + (i + 0.5) * bsz / g``, the strict ``v < -1`` / ``v > size`` tests, the clamps at 0 and
    ``size - 1``, the level formula).  These are discrete decisions: in float64 they would be a different function exactly
    at the edges the tests are about (a sample ON -1 or ON ``size``, a coordinate that rounds onto an integer);
  * the WEIGHTS (products of the float32 ``l`` and ``h = 1 - l``) and every sum are float64.

Only the trailing axes of the feature arrays are vectorised (channels; a caller may stack images in front of them).
Besides the pooled values every call returns what it decided, per box and axis: ``g``, the samples it skipped and the
number of distinct feature pixels each bin touched -- ``tests/roi_align_cases.py`` is checked against these.
"""
import numpy as np

f32 = np.float32

STRIDES = (4, 8, 16, 32)          # p2 .. p5


def level_value(box) -> np.float32:
    """``4 + log2(sqrt(area) / 224 + 1e-8)`` in float32, before floor and clamp."""
    x1, y1, x2, y2 = (f32(v) for v in box)
    area = (x2 - x1) * (y2 - y1)
    return f32(4.0) + np.log2(np.sqrt(area) / f32(224.0) + f32(1e-8))


def assign_level(box) -> int:
    """Index 0 .. 3 into (p2, p3, p4, p5)."""
    lv = np.floor(level_value(box))
    lv = min(max(lv, f32(2.0)), f32(5.0))
    return int(lv) - 2


def level_is_unambiguous(box, margin: float = 1e-4) -> bool:
    """False where another rounding of sqrt / log2 could put the box on the other side of a boundary between two levels
    (3, 4 and 5 before the clamp: below 3 everything is p2, from 5 on everything p5)."""
    x1, y1, x2, y2 = (float(f32(v)) for v in box)
    area = (x2 - x1) * (y2 - y1)
    if area < 0.0:
        return False
    v = 4.0 + np.log2(np.sqrt(area) / 224.0 + 1e-8)
    return all(abs(v - edge) > margin for edge in (3.0, 4.0, 5.0))


def axis_samples(c1, c2, scale, P: int, size: int):
    """One axis of one box.  Returns ``g`` and, per bin, the list of its samples as ``(v, kept, lo, hi, l, h)`` with ``v`` the
    raw float32 coordinate (before any clamp) and ``l``, ``h`` float32."""
    scale = f32(scale)
    start = f32(c1) * scale - f32(0.5)
    end = f32(c2) * scale - f32(0.5)
    ext = end - start
    bsz = ext / f32(P)
    g = int(np.ceil(ext / f32(P)))
    bins = []
    for b in range(P):
        samples = []
        for i in range(max(g, 0)):
            v = start + f32(b) * bsz + (f32(i) + f32(0.5)) * bsz / f32(g)
            raw = v
            if v < f32(-1.0) or v > f32(size):
                samples.append((raw, False, 0, 0, f32(0.0), f32(0.0)))
                continue
            if v <= f32(0.0):
                v = f32(0.0)
            lo = int(v)
            if lo >= size - 1:
                lo = hi = size - 1
                v = f32(lo)
            else:
                hi = lo + 1
            l = v - f32(lo)
            h = f32(1.0) - l
            samples.append((raw, True, lo, hi, l, h))
        bins.append(samples)
    return g, bins


def _axis_diag(g, bins):
    return {
        "g": g,
        "skipped": sum(1 for s in bins for t in s if not t[1]),
        "touched": [len({p for t in s if t[1] for p in (t[2], t[3])}) for s in bins],
        "coords": [[float(t[0]) for t in s] for s in bins],
    }


def box_diag(box, P: int, sizes) -> dict:
    """The decisions alone.  ``sizes``: (H, W) of the four levels."""
    lv = assign_level(box)
    H, W = sizes[lv]
    scale = f32(1.0) / f32(STRIDES[lv])
    gy, by = axis_samples(box[1], box[3], scale, P, H)
    gx, bx = axis_samples(box[0], box[2], scale, P, W)
    return {"level": lv, "y": _axis_diag(gy, by), "x": _axis_diag(gx, bx)}


def roi_align_box(levels, box, P: int):
    """``levels``: four arrays [H, W, ...] (p2 .. p5), any float type; ``box``: (x1, y1, x2, y2).  Returns the pooled
    [P, P, ...] in float64 and the diagnostics of ``box_diag``."""
    lv = assign_level(box)
    feat = levels[lv]
    H, W = feat.shape[:2]
    scale = f32(1.0) / f32(STRIDES[lv])
    gy, by = axis_samples(box[1], box[3], scale, P, H)
    gx, bx = axis_samples(box[0], box[2], scale, P, W)
    out = np.zeros((P, P) + feat.shape[2:], dtype=np.float64)
    count = float(max(gy * gx, 1))
    for ph in range(P):
        for pw in range(P):
            acc = np.zeros(feat.shape[2:], dtype=np.float64)
            for (_, ky, yl, yh, ly, hy) in by[ph]:
                if not ky:
                    continue
                ly, hy = float(ly), float(hy)
                for (_, kx, xl, xh, lx, hx) in bx[pw]:
                    if not kx:
                        continue
                    lx, hx = float(lx), float(hx)
                    acc += (hy * hx) * feat[yl, xl].astype(np.float64)
                    acc += (hy * lx) * feat[yl, xh].astype(np.float64)
                    acc += (ly * hx) * feat[yh, xl].astype(np.float64)
                    acc += (ly * lx) * feat[yh, xh].astype(np.float64)
            out[ph, pw] = acc / count
    return out, {"level": lv, "y": _axis_diag(gy, by), "x": _axis_diag(gx, bx)}


def roi_pool(levels, boxes, P: int):
    """All boxes of one table: [R, P, P, ...] float64, the list of diagnostics."""
    outs, diags = [], []
    for box in boxes:
        o, d = roi_align_box(levels, box, P)
        outs.append(o)
        diags.append(d)
    return np.stack(outs), diags
