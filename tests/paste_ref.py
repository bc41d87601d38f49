"""An independent reference of the mask paste (``demia_paste_masks``, csrc/paste.hip) in numpy: the box contract in float32,
the sampling in float64.  It shares no code with the kernel or with ``oracle/maskrcnn_ref.py``; the sampling is written as
two small matrices of tap weights (one per axis) around the 28 x 28 mask, not as a per-pixel gather.

  * ``out_boxes``: detection boxes -> output-frame boxes, the f32 contract (scale, clip, validity), meant to be bit-exact;
  * ``window``: the pixels a valid box may set;
  * ``paste64``: the f64 probability of every pixel of the frame for one f32 box;
  * ``blocked_mask_prob``: [n, 28, 28] masks + class ids -> the mask head's blocked output layout;
  * ``pack_bits`` / ``unpack_bits`` / ``tight_box``: the packed-mask layout on the host.
"""
import math

import numpy as np

MASK = 28
CELLS = 196
F32 = np.float32


def out_boxes(det_boxes, img_h: int, img_w: int, out_h: int, out_w: int):
    """[..., 4] boxes (x0, y0, x1, y1) of the network's frame -> (f32 boxes of the output frame, validity).  Every operation
    is one float32 operation: the scale is ``float32(out / img)`` (the quotient taken in double), x is clipped to
    [0, out_w] and y to [0, out_h], and a box is valid when its f32 width and height are both > 0."""
    b = np.asarray(det_boxes, dtype=F32)
    scale = (F32(out_w / img_w), F32(out_h / img_h))
    limit = (F32(out_w), F32(out_h))
    ob = np.empty_like(b)
    for k in range(4):
        ob[..., k] = np.minimum(np.maximum(b[..., k] * scale[k & 1], F32(0.0)), limit[k & 1])
    valid = ((ob[..., 2] - ob[..., 0]) > F32(0.0)) & ((ob[..., 3] - ob[..., 1]) > F32(0.0))
    return ob, valid


def window(box, H: int, W: int):
    """(y0, x0, y1, x1), ends exclusive: [max(floor(lo) - 1, 0), min(ceil(hi) + 1, size)) on each axis."""
    x0, y0, x1, y1 = (float(v) for v in box)
    return (max(math.floor(y0) - 1, 0), max(math.floor(x0) - 1, 0), min(math.ceil(y1) + 1, H), min(math.ceil(x1) + 1, W))


def hint_of(win):
    """The window in the inclusive form the kernel reports (``out_bbox``)."""
    return (win[0], win[1], win[2] - 1, win[3] - 1)


def _axis_weights(lo: int, hi: int, a0: float, a1: float) -> np.ndarray:
    """[hi - lo, 28] float64: row p holds the bilinear weights of pixel lo + p on the 28 mask cells of this axis.  The sample
    position of pixel c is (c + 0.5 - a0) / (a1 - a0) * 28 - 0.5 in cell units (cell k has its centre at k); a tap outside
    0 .. 27 reads zero padding, so its weight is simply left out."""
    c = np.arange(lo, hi, dtype=np.float64) + 0.5
    t = (c - a0) / (a1 - a0) * MASK - 0.5
    f = np.floor(t)
    w = t - f
    A = np.zeros((hi - lo, MASK), dtype=np.float64)
    for tap, wt in ((f, 1.0 - w), (f + 1.0, w)):
        ok = (tap >= 0) & (tap <= MASK - 1)
        A[np.nonzero(ok)[0], tap[ok].astype(np.int64)] += wt[ok]
    return A


def paste64(mask28, box_f32, H: int, W: int):
    """(plane [H, W] float64, window): the bilinear sample (zero padding, pixel centres at +0.5) of the 28 x 28 mask stretched
    over the f32 box, at every pixel of the box's window; zero outside the window.  A pixel is set when plane >= 0.5."""
    x0, y0, x1, y1 = (float(v) for v in np.asarray(box_f32, dtype=F32))
    win = window((x0, y0, x1, y1), H, W)
    plane = np.zeros((H, W), dtype=np.float64)
    wy0, wx0, wy1, wx1 = win
    if wy1 > wy0 and wx1 > wx0:
        Ay = _axis_weights(wy0, wy1, y0, y1)
        Ax = _axis_weights(wx0, wx1, x0, x1)
        plane[wy0:wy1, wx0:wx1] = Ay @ np.asarray(mask28, dtype=np.float64) @ Ax.T
    return plane, win


def blocked_mask_prob(masks, classes, K: int, wrong: float = -1.0, pad: float = 7.0) -> np.ndarray:
    """[n, 28, 28] masks, [n] class ids -> float32 [n * 196 * 4, ld], row (inst * 196 + cell) * 4 + sub with
    cell = (y >> 1) * 14 + (x >> 1), sub = (y & 1) * 2 + (x & 1), ld = K rounded up to a multiple of 4.  The instance's own
    class column holds its mask; every other class column ``wrong`` (reading it empties the mask) and every padding column
    ``pad`` (reading it fills the window)."""
    masks = np.asarray(masks, dtype=F32)
    classes = np.asarray(classes, dtype=np.int64)
    n = masks.shape[0]
    ld = (K + 3) // 4 * 4
    out = np.full((n, CELLS, 4, ld), pad, dtype=F32)
    out[..., :K] = wrong
    inst = np.arange(n)[:, None]
    cell = np.arange(CELLS)[None, :]
    for dy in range(2):
        for dx in range(2):
            out[inst, cell, dy * 2 + dx, classes[:, None]] = masks[:, dy::2, dx::2].reshape(n, CELLS)
    return out.reshape(n * CELLS * 4, ld)


def pack_bits(dense) -> np.ndarray:
    """bool [..., H, W] -> uint32 [..., H, ceil(W / 32)]: pixel x is bit (x & 31) of word (x >> 5); padding bits zero."""
    dense = np.asarray(dense, dtype=bool)
    W = dense.shape[-1]
    wpr = (W + 31) // 32
    padded = np.zeros(dense.shape[:-1] + (wpr * 32,), dtype=bool)
    padded[..., :W] = dense
    return np.ascontiguousarray(np.packbits(padded, axis=-1, bitorder="little")).view(np.uint32)


def unpack_bits(words, W: int) -> np.ndarray:
    """The inverse of ``pack_bits``, padding bits INCLUDED: bool [..., H, 32 * wpr] (slice [..., :W] for the frame)."""
    words = np.ascontiguousarray(np.asarray(words).view(np.uint32))
    return np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little").astype(bool)


def tight_box(dense):
    """(area, [y0, x0, y1, x1] inclusive) of one bool plane; the box is -1 when the plane is empty."""
    ys, xs = np.nonzero(dense)
    if len(ys) == 0:
        return 0, [-1, -1, -1, -1]
    return int(len(ys)), [int(ys.min()), int(xs.min()), int(ys.max()), int(xs.max())]
