"""CPU statements of the boundary band (``include/deepemia_hip.h``: demia_mask_boundary_band), independent of the kernel's bit-row
scheme:

``eroded_literal``    the definition, pixel by pixel and window by window (small frames only);
``eroded``            the same predicate for whole stacks: a pixel survives iff its (2d + 1)^2 window, read from the mask padded
                      with d zeros all around, holds (2d + 1)^2 ones -- counted with a summed-area table in int64;
``eroded_published``  the published construction (Cheng et al., Boundary IoU, CVPR 2021): a 1-px zero ring, then d iterations of a
                      3 x 3 erosion whose own border counts as set (``scipy.ndimage.binary_erosion``);
``band``              ``m & ~eroded(m, d)``;
``boundary_iou``      on dense arrays: ``|band(a) & band(g)| / (|band(a)| + |band(g)| - |band(a) & band(g)|)``, the denominator
                      ``|band(a)|`` for a crowd ground truth, 0 where the bands do not meet.
"""
import numpy as np


def eroded_literal(m, d):
    m = np.asarray(m, dtype=bool)
    H, W = m.shape
    out = np.zeros((H, W), dtype=bool)
    for y in range(H):
        for x in range(W):
            ok = True
            for j in range(-d, d + 1):
                for i in range(-d, d + 1):
                    yy, xx = y + j, x + i
                    if yy < 0 or yy >= H or xx < 0 or xx >= W or not m[yy, xx]:
                        ok = False
                        break
                if not ok:
                    break
            out[y, x] = ok
    return out


def eroded(m, d):
    """[..., H, W] bool -> the erosion by the (2d + 1) x (2d + 1) square, outside the frame = 0."""
    m = np.asarray(m, dtype=bool)
    H, W = m.shape[-2:]
    d = int(d)
    if 2 * d + 1 > H or 2 * d + 1 > W:          # no window lies inside the frame
        return np.zeros_like(m)
    n = 2 * d + 1
    pad = [(0, 0)] * (m.ndim - 2) + [(d + 1, d), (d + 1, d)]           # one more row / column in front for the table's zero edge
    s = np.pad(m, pad).astype(np.int64).cumsum(-2).cumsum(-1)
    cnt = s[..., n:, n:] - s[..., :-n, n:] - s[..., n:, :-n] + s[..., :-n, :-n]
    assert cnt.shape == m.shape
    return cnt == n * n


def eroded_published(m, d):
    from scipy import ndimage

    m = np.asarray(m, dtype=bool)
    lead = m.ndim - 2
    padded = np.pad(m, [(0, 0)] * lead + [(1, 1), (1, 1)])
    st = np.ones((1,) * lead + (3, 3), dtype=bool)
    out = ndimage.binary_erosion(padded, structure=st, iterations=int(d), border_value=1)
    return out[..., 1:-1, 1:-1]


def band(m, d):
    m = np.asarray(m, dtype=bool)
    return m & ~eroded(m, d)


def boundary_iou(a, g, d, crowd=False):
    ba, bg = band(a, d), band(g, d)
    i = int(np.count_nonzero(ba & bg))
    if i == 0:
        return 0.0
    u = int(ba.sum()) if crowd else int(ba.sum()) + int(bg.sum()) - i
    return i / u


def mask_iou(a, g, crowd=False):
    a, g = np.asarray(a, dtype=bool), np.asarray(g, dtype=bool)
    i = int(np.count_nonzero(a & g))
    if i == 0:
        return 0.0
    return i / (int(a.sum()) if crowd else int(a.sum()) + int(g.sum()) - i)


def tight_box(m):
    ys, xs = np.nonzero(m)
    return [int(ys.min()), int(xs.min()), int(ys.max()), int(xs.max())] if len(ys) else [-1] * 4
