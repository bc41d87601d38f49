"""An exact reference of the ten values ``demia_contour_shape`` writes per contour, sharing no code with the kernel:

* the hull is a monotone chain in Python ``int`` (arbitrary precision);
* ``F2`` and the tie rule of the max-Feret pair come from brute force over ALL pairs of points, not over hull vertices
  (vectorised int64 numpy, block by block, for large n);
* ``MinFeret`` goes over hull edges x hull vertices with the cross products in Python ``int`` and one float64 quotient;
* the hull perimeter is summed with ``math.fsum``.

Values 0-2 are exact integers; the others are a handful of correctly rounded float64 operations on exact integers.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np

SHAPE_COLS = 10
SHAPE_KEYS = ("S2", "F2", "k", "Convex area", "Convex perimeter", "Solidity", "Convexity", "Max Feret diameter", "Min Feret diameter",
              "Feret angle")
REL_TOL = 1e-12          # values 3..8, relative
ANGLE_TOL = 1e-9         # value 9, degrees


def hull(points) -> List[Tuple[int, int]]:
    """Strict convex hull of the distinct points, counter-clockwise in (x, y): 1 vertex for one distinct point, 2 for collinear
    points, else >= 3.  Collinear points are no vertices."""
    p = sorted({(int(x), int(y)) for x, y in np.asarray(points).reshape(-1, 2).tolist()})
    if len(p) <= 2:
        return p

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    lower: List[Tuple[int, int]] = []
    for q in p:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], q) <= 0:
            lower.pop()
        lower.append(q)
    upper: List[Tuple[int, int]] = []
    for q in reversed(p):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], q) <= 0:
            upper.pop()
        upper.append(q)
    return lower[:-1] + upper[:-1]


def farthest_pair(points) -> Tuple[int, Tuple[int, int], Tuple[int, int]]:
    """(F2, a, b): the largest squared distance between two points, and among the pairs that have it -- each ordered so that
    a < b by (x, y) -- the one with the smallest a, then the smallest b.  Brute force over all pairs of distinct points."""
    p = np.unique(np.asarray(points, dtype=np.int64).reshape(-1, 2), axis=0)          # sorted by (x, y)
    n = len(p)
    if n == 1:
        return 0, (int(p[0, 0]), int(p[0, 1])), (int(p[0, 0]), int(p[0, 1]))
    best = -1
    pair = None
    step = max(1, (1 << 22) // n)
    for i0 in range(0, n, step):
        d = p[i0:i0 + step, None, :] - p[None, :, :]
        d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]
        top = int(d2.max())
        if top < best:
            continue
        ii, jj = np.nonzero(d2 == top)
        ii = ii + i0
        lo, hi = np.minimum(ii, jj), np.maximum(ii, jj)                                # sorted order: index order IS (x, y) order
        k = np.lexsort((hi, lo))[0]
        cand = (int(lo[k]), int(hi[k]))
        if top > best or cand < pair:
            best, pair = top, cand
    return best, (int(p[pair[0], 0]), int(p[pair[0], 1])), (int(p[pair[1], 0]), int(p[pair[1], 1]))


def min_feret(h: Sequence[Tuple[int, int]]) -> float:
    if len(h) < 3:
        return 0.0
    best = math.inf
    for i in range(len(h)):
        a, b = h[i], h[(i + 1) % len(h)]
        ex, ey = b[0] - a[0], b[1] - a[1]
        far = max(abs(ex * (v[1] - a[1]) - ey * (v[0] - a[0])) for v in h)
        best = min(best, far / math.sqrt(ex * ex + ey * ey))
    return best


def shape_values(points, area: float, perimeter: float, um: float) -> np.ndarray:
    """The ten values for one contour; ``area`` / ``perimeter``: its contourArea / arcLength (``red``)."""
    h = hull(points)
    k = len(h)
    s2 = 0
    if k >= 3:
        s2 = abs(sum(h[i][0] * h[(i + 1) % k][1] - h[(i + 1) % k][0] * h[i][1] for i in range(k)))
    if k == 1:
        ph = 0.0
    else:
        ph = math.fsum(math.sqrt((h[(i + 1) % k][0] - h[i][0]) ** 2 + (h[(i + 1) % k][1] - h[i][1]) ** 2) for i in range(k))
    f2, a, b = farthest_pair(points)
    angle = 0.0
    if f2 > 0:
        angle = math.degrees(math.atan2(-(b[1] - a[1]), b[0] - a[0]))
        if angle < 0:
            angle += 180.0
        if angle >= 180.0:
            angle = 0.0
    return np.array([float(s2), float(f2), float(k), s2 / 2 * um * um, ph * um, area / (s2 / 2) if s2 else 0.0,
                     ph / perimeter if perimeter else 0.0, math.sqrt(f2) * um, min_feret(h) * um, angle], dtype=np.float64)


def compare(got, want) -> List[str]:
    """Everything wrong with the kernel's ten values ``got`` against the reference's ``want``."""
    bad = []
    for j in range(3):
        if got[j] != want[j]:
            bad.append(f"{SHAPE_KEYS[j]}: {got[j]!r} != {want[j]!r} (must be exact)")
    for j in range(3, 9):
        if abs(got[j] - want[j]) > REL_TOL * abs(want[j]):
            bad.append(f"{SHAPE_KEYS[j]}: {got[j]!r} != {want[j]!r} (rel {abs(got[j] - want[j]) / max(abs(want[j]), 1e-300):.3g})")
    if abs(got[9] - want[9]) > ANGLE_TOL:
        bad.append(f"{SHAPE_KEYS[9]}: {got[9]!r} != {want[9]!r}")
    return bad


def spur_contour() -> np.ndarray:
    """A 12 x 8 rectangle as CHAIN_APPROX_SIMPLE leaves it, with a 1-px wide spur of 5 px on its top side: the walk goes out to
    the tip and back, so the spur's foot appears twice."""
    return np.array([[40, 30], [40, 37], [51, 37], [51, 30], [46, 30], [46, 25], [46, 30]], dtype=np.int32) + np.array([900, 700], dtype=np.int32)
