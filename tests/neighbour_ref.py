"""A literal reference of the neighbour statistics (``demia_mask_neighbours``; definition: ``include/deepemia_hip.h``) on dense
NumPy masks, with Python-int results.

``d2(a, b)`` is the smallest squared distance between a pixel centre of a and one of b.  Two ways to it that share nothing with
the kernels (no borders, no boxes, no pruning): brute force over all coordinate pairs (``pair_d2_brute``), and, for the larger
scenes, the nearest pixel of b for EVERY pixel of the frame from ``scipy.ndimage.distance_transform_edt``'s index output, from
which the squared distance is recomputed in integers (``d2_matrix``) -- exact, no rounding of a float distance.
"""
import numpy as np
from scipy import ndimage

NONE = -1


def pair_d2_brute(a: np.ndarray, b: np.ndarray) -> int:
    """min (px - qx)^2 + (py - qy)^2 over the set pixels of a and b, all pairs; -1 when either is empty."""
    ay, ax = np.nonzero(a)
    by, bx = np.nonzero(b)
    if len(ay) == 0 or len(by) == 0:
        return NONE
    best = None
    for s in range(0, len(ay), 2048):                 # (chunks: the pair table of two large masks would not fit)
        dy = ay[s:s + 2048, None].astype(np.int64) - by[None, :].astype(np.int64)
        dx = ax[s:s + 2048, None].astype(np.int64) - bx[None, :].astype(np.int64)
        m = int((dy * dy + dx * dx).min())
        best = m if best is None else min(best, m)
    return best


def d2_matrix(masks: np.ndarray) -> list:
    """[M][M] Python ints: d2(a, b); -1 on the diagonal and where a or b is empty."""
    masks = np.asarray(masks) != 0
    M = masks.shape[0]
    out = [[NONE] * M for _ in range(M)]
    coords = [np.nonzero(m) for m in masks]
    filled = [k for k in range(M) if len(coords[k][0])]
    if not filled:
        return out
    ys = np.concatenate([coords[k][0] for k in filled]).astype(np.int64)
    xs = np.concatenate([coords[k][1] for k in filled]).astype(np.int64)
    starts = np.cumsum([0] + [len(coords[k][0]) for k in filled[:-1]])
    for b in filled:
        iy, ix = ndimage.distance_transform_edt(~masks[b], return_distances=False, return_indices=True)
        dy, dx = iy[ys, xs].astype(np.int64) - ys, ix[ys, xs].astype(np.int64) - xs
        col = np.minimum.reduceat(dy * dy + dx * dx, starts)
        for a, v in zip(filled, col.tolist()):
            if a != b:
                out[a][b] = int(v)
    return out


def sums(masks: np.ndarray) -> list:
    """[M][3] Python ints: N, Sx, Sy."""
    out = []
    for m in np.asarray(masks) != 0:
        y, x = np.nonzero(m)
        out.append([int(len(y)), int(x.astype(np.int64).sum()), int(y.astype(np.int64).sum())])
    return out


def table(masks: np.ndarray, group=None, r2: int = -1, d2=None) -> list:
    """[M][6] Python ints: d2_any, idx_any, d2_group, idx_group, touching, within -- the nearest b != a with a pixel by (d2, b),
    the lower index winning a tie; the same among the masks of a's group; the count of b with d2 <= 2; the count with d2 <= r2
    (-1 for r2 < 0).  A mask without a pixel: -1, -1, -1, -1, 0, within (0 or -1)."""
    masks = np.asarray(masks) != 0
    M = masks.shape[0]
    d2 = d2_matrix(masks) if d2 is None else d2
    n = [int(m.sum()) for m in masks]
    group = [0] * M if group is None else [int(g) for g in group]
    rows = []
    for a in range(M):
        within = NONE if r2 < 0 else 0
        if n[a] == 0:
            rows.append([NONE, NONE, NONE, NONE, 0, within])
            continue
        best, best_g, touching = None, None, 0
        for b in range(M):
            if b == a or n[b] == 0:
                continue
            d = d2[a][b]
            assert d >= 0
            if best is None or (d, b) < best:
                best = (d, b)
            if group[b] == group[a] and (best_g is None or (d, b) < best_g):
                best_g = (d, b)
            touching += d <= 2
            if r2 >= 0:
                within += d <= r2
        rows.append(list(best or (NONE, NONE)) + list(best_g or (NONE, NONE)) + [int(touching), int(within)])
    return rows


def border(mask: np.ndarray) -> set:
    """{(y, x)}: the set pixels with an unset 4-neighbour, positions outside the frame counting as unset."""
    m = np.asarray(mask) != 0
    p = np.pad(m, 1)
    inner = p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    y, x = np.nonzero(m & ~inner)
    return set(zip(y.tolist(), x.tolist()))


def tight_boxes(masks: np.ndarray) -> np.ndarray:
    """[M, 4] int32 (y0, x0, y1, x1), inclusive; -1 for a mask without a pixel."""
    out = np.full((len(masks), 4), -1, dtype=np.int32)
    for k, m in enumerate(np.asarray(masks) != 0):
        y, x = np.nonzero(m)
        if len(y):
            out[k] = (y.min(), x.min(), y.max(), x.max())
    return out
