"""What ``test_cpu_contour_geometry.py`` and ``test_gpu_contour_measure.py`` share: the seeded contour cases, the tables that
``demia_contour_measure`` reads (built from plain point lists, no tracer involved), its launch, and a float64 reference of the
twelve measurement values that shares no code with ``oracle/postproc_ref.py`` except ``order_points`` (whose semantics
``test_cpu_oracle_postproc_goldens.py::test_order_points_and_box_points`` pins).

The reference is geometry, not a restatement of OpenCV:

* minimum-area rectangle: hull vertices from ``scipy.spatial.ConvexHull``; a minimal enclosing rectangle has a side on a hull
  edge, so every edge's rectangle is computed in float64 and the smallest kept (no calipers, no Sklansky scan);
* the product then truncates the four corners to int and orders them -- a discontinuous step, so the reference is SET-valued:
  a corner coordinate within ``SNAP`` of an integer may fall on either side (at most 2^8 candidates);
* ellipse: centred and scaled float64 points, ``numpy.linalg.lstsq`` for the five-parameter conic, ``solve`` for its centre,
  ``lstsq`` for the three-parameter form about that centre, axes from the eigenvalues of the 2 x 2 form (no Jacobi SVD);
* the four area / perimeter values by closed form.

Nothing in here needs a GPU except :func:`measure_tables`.
"""
from __future__ import annotations

import itertools
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

KEYS = ("major_axis_length", "minor_axis_length", "eccentricity", "Length", "Width", "CircularED", "Aspect_Ratio",
        "Circularity", "Chords", "Feret_diam", "Roundness", "Sphericity")      # order of demia_contour_measure's 12 values
ELLIPSE_IDX = (0, 1, 2)
UM = 0.37

SNAP = 1e-3              # a corner coordinate this close to an integer may truncate to either side
RECT_TOL = 1e-6          # (Length, Width) must equal one candidate within RECT_TOL * um_pix
TIE_AREA = 1e-6          # a second rectangle within this relative area ...
TIE_SIDE = 1e-9          # ... whose sides differ by more than this (relative) makes the case ill-posed
CLOSED_TOL = 1e-12       # relative, area / perimeter values against closed form

# Ellipse values, relative: four times the worst difference between the oracle and the float64 reference below, measured on
# the CPU over all cases of test_cpu_contour_geometry.py (figures in that module's header).  Never measured on the kernel.
ELLIPSE_WORST_SMALL_N = 1.53e-6          # n < 10: exactly or nearly determined fits amplify the f32 centroid and output rounding
ELLIPSE_WORST = 2.34e-7                  # n >= 10 (a traced 55-point rectangle at frame offset (16000, 15000): f32 centroid sums)
ELLIPSE_BOUND_SMALL_N = 4 * ELLIPSE_WORST_SMALL_N
ELLIPSE_BOUND = 4 * ELLIPSE_WORST
# The oracle (as the reference program) takes the midpoint distances in float32: squares and their sum round once each, the
# root halves it, so its Length / Width sit within one float32 epsilon (relative) of the float64 value.  The kernel computes
# them in float64 and gets no such allowance.
ORACLE_F32 = 2.0 ** -23

SIZES = (5, 6, 7, 9, 33, 64, 65, 255, 256, 257, 1000, 4096, 4097, 6000)
SEED = 20240611


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    points: np.ndarray           # (n, 2) int32, (x, y)

    @property
    def n(self) -> int:
        return int(self.points.shape[0])


def noisy_ellipse(rng: np.random.Generator, n: int) -> np.ndarray:
    """n points on a rotated ellipse at sorted random angles, 3 % radial noise, rounded to int32: never axis-aligned, never
    symmetric.  Small contours stay small (n < 40); frame offsets reach 15000."""
    if n < 40:
        a = rng.uniform(8.0, 30.0)
    elif n < 4000:
        a = rng.uniform(60.0, 600.0)
    else:
        a = rng.uniform(600.0, 1500.0)
    b = a * rng.uniform(0.35, 0.8)
    th = np.sort(rng.uniform(0.0, 2.0 * math.pi, n))
    r = 1.0 + 0.03 * rng.standard_normal(n)
    rot = rng.uniform(0.1, 1.4)
    x, y = a * np.cos(th) * r, b * np.sin(th) * r
    c, s = math.cos(rot), math.sin(rot)
    ox, oy = rng.uniform(2.0 * a + 8.0, 15000.0, 2)
    pts = np.stack([ox + c * x - s * y, oy + s * x + c * y], axis=1)
    return np.rint(pts).astype(np.int32)


_CASES: Optional[List[Case]] = None


def generated_cases() -> List[Case]:
    """Three repetitions of every size below 4000 points, one of 4096, 4097 and 6000: 36 cases, the same on every call."""
    global _CASES
    if _CASES is None:
        rng = np.random.default_rng(SEED)
        out = []
        for n in SIZES:
            for rep in range(3 if n < 4000 else 1):
                out.append(Case(f"n{n}_r{rep}", noisy_ellipse(rng, n)))
        _CASES = out
    return _CASES


def traced_masks() -> List[Tuple[str, np.ndarray]]:
    """Rotated rectangles and rough ellipses, 30 to 700 px long, one connected shape per mask."""
    out = []
    for k, size in enumerate((30, 75, 200, 700)):
        side = int(size * 1.3) + 8
        yy, xx = np.mgrid[0:side, 0:side].astype(np.float64)
        cx = cy = side / 2.0 + 0.3
        for kind, rot in (("rect", 0.35 + 0.27 * k), ("ellipse", 1.2 - 0.31 * k)):
            c, s = math.cos(rot), math.sin(rot)
            u, v = (xx - cx) * c + (yy - cy) * s, -(xx - cx) * s + (yy - cy) * c
            if kind == "rect":
                m = (np.abs(u) <= size / 2.0) & (np.abs(v) <= size * (0.2 + 0.05 * k))
            else:
                ang = np.arctan2(v, u)
                rough = 1.0 + 0.06 * np.sin(5 * ang + k) + 0.03 * np.sin(11 * ang)
                m = (u / (size / 2.0)) ** 2 + (v / (size * (0.17 + 0.06 * k))) ** 2 <= rough ** 2
            out.append((f"{kind}{size}", m))
    return out


def traced_cases() -> List[Case]:
    """The external contour of every :func:`traced_masks` shape as the oracle's tracer gives it, in place and moved by the
    frame offset (16000, 15000)."""
    from oracle import postproc_ref as P

    out = []
    for name, m in traced_masks():
        cs = P.find_external_contours(m)
        assert len(cs) == 1, (name, len(cs))
        out.append(Case(name, cs[0].astype(np.int32)))
        out.append(Case(name + "_far", (cs[0] + np.array([16000, 15000])).astype(np.int32)))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# float64 reference
# ----------------------------------------------------------------------------------------------------------------------
class IllPosed(AssertionError):
    """The case has no single right answer (two different minimal rectangles, a conic that is no ellipse)."""


def hull_vertices(points: np.ndarray) -> np.ndarray:
    """Vertices of the convex hull, float64 (k, 2): k = 1 for one distinct point, k = 2 (the two ends) for collinear points."""
    p = np.unique(np.asarray(points, dtype=np.int64).reshape(-1, 2), axis=0)
    if len(p) == 1:
        return p.astype(np.float64)
    d = p - p[0]
    k = int(np.argmax((d * d).sum(axis=1)))
    if not np.any(d[:, 0] * d[k, 1] - d[:, 1] * d[k, 0]):             # exact in int64: every point on the line p[0] -> p[k]
        t = d @ d[k]
        return p[[int(np.argmin(t)), int(np.argmax(t))]].astype(np.float64)
    from scipy.spatial import ConvexHull

    return p[ConvexHull(p.astype(np.float64)).vertices].astype(np.float64)


def min_area_rectangles(points: np.ndarray, ties: str = "raise") -> List[np.ndarray]:
    """The four corners (float64, going round) of the smallest enclosing rectangle.  A tie between rectangles of different
    side lengths raises :class:`IllPosed`, or with ``ties="all"`` returns every tied rectangle (a triangle always ties: the
    rectangle on each of its sides has twice its area)."""
    h = hull_vertices(points)
    if len(h) == 1:
        return [np.repeat(h, 4, axis=0)]
    if len(h) == 2:                                                     # zero height: every corner is one of the two ends
        return [np.array([h[0], h[0], h[1], h[1]])]
    rects = []
    for i in range(len(h)):
        e = h[(i + 1) % len(h)] - h[i]
        u = e / math.hypot(e[0], e[1])
        v = np.array([-u[1], u[0]])
        pu, pv = h @ u, h @ v
        rects.append((float((pu.max() - pu.min()) * (pv.max() - pv.min())), pu.min(), pu.max(), pv.min(), pv.max(), u, v))
    best = min(rects, key=lambda r: r[0])
    sides = sorted((best[2] - best[1], best[4] - best[3]))
    out = [best]
    for r in rects:
        if r is not best and r[0] - best[0] <= TIE_AREA * best[0]:
            s = sorted((r[2] - r[1], r[4] - r[3]))
            if abs(s[0] - sides[0]) > TIE_SIDE * sides[1] or abs(s[1] - sides[1]) > TIE_SIDE * sides[1]:
                if ties != "all":
                    raise IllPosed(f"two minimal rectangles: sides {sides} and {s}, areas {best[0]!r} and {r[0]!r}")
                out.append(r)
    return [np.array([u0 * u + v0 * v, u1 * u + v0 * v, u1 * u + v1 * v, u0 * u + v1 * v]) for _, u0, u1, v0, v1, u, v in out]


def _length_width(box: np.ndarray, um: float) -> Tuple[float, float]:
    """Truncated corners -> order_points -> distances between the midpoints of opposite sides, in float64."""
    from oracle.postproc_ref import order_points

    tl, tr, br, bl = order_points(box).astype(np.float64)
    d_a = float(np.hypot(*((tl + tr) * 0.5 - (bl + br) * 0.5)))
    d_b = float(np.hypot(*((tl + bl) * 0.5 - (tr + br) * 0.5)))
    return min(d_a, d_b) * um, max(d_a, d_b) * um


def rect_candidates(points: np.ndarray, um: float = UM, ties: str = "raise") -> List[Tuple[float, float]]:
    """Every (Length, Width) that a correct minimal rectangle can give after the int truncation of its corners."""
    if len(hull_vertices(points)) == 1:
        return [(0.0, 0.0)]                    # the rectangle IS the integer point: nothing is computed, nothing can truncate
    out = []
    for rect in min_area_rectangles(points, ties):
        opts = []
        for v in rect.reshape(-1):
            if abs(v - round(v)) <= SNAP:
                opts.append(sorted({int(v - SNAP), int(v + SNAP)}))
            else:
                opts.append([int(v)])
        for combo in itertools.product(*opts):
            lw = _length_width(np.array(combo, dtype=np.int64).reshape(4, 2), um)
            if lw not in out:
                out.append(lw)
    return out


def rect_derived(length: float, width: float, um: float = UM) -> dict:
    """The five rectangle values that follow from (Length, Width) (index into the 12 -> value)."""
    aspect = width / length if length != 0 and width != 0 else 0.0
    return {3: length, 4: width, 6: aspect, 9: width, 10: 1.0 / aspect if aspect != 0 else 0.0}


def match_rect(values: Sequence[float], points: np.ndarray, um: float = UM, rel: float = 0.0, ties: str = "raise") -> Optional[str]:
    """None when ``values`` (12) agree with one rectangle candidate, else what is wrong.  ``rel``: relative allowance on top
    of ``RECT_TOL * um`` for a float32 implementation (``ORACLE_F32`` for the oracle, 0 for the kernel)."""
    cands = rect_candidates(points, um, ties)
    for length, width in cands:
        if abs(values[3] - length) <= RECT_TOL * um + rel * length and abs(values[4] - width) <= RECT_TOL * um + rel * width:
            for j, e in rect_derived(length, width, um).items():
                # candidates differ by whole pixels, so a matched (Length, Width) came from the same four int corners: the
                # quotients Aspect and Roundness then agree to rounding
                if abs(values[j] - e) > (RECT_TOL * um + rel * e if j in (3, 4, 9) else (CLOSED_TOL + 2 * rel) * abs(e)):
                    return f"{KEYS[j]} {values[j]!r} != {e!r} (from Length {length!r}, Width {width!r})"
            return None
    return f"(Length, Width) = ({values[3]!r}, {values[4]!r}) is none of the {len(cands)} candidates {cands[:4]}"


def ref_ellipse(points: np.ndarray, um: float = UM) -> Tuple[float, float, float]:
    """(shorter axis, longer axis, eccentricity) of the algebraic least-squares ellipse, the two full axes times ``um``."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    n = len(p)
    q = p - p.mean(axis=0)
    k = 100.0 / np.abs(q).sum()
    x, y = (q * k).T
    g = np.linalg.lstsq(np.stack([-x * x, -y * y, -x * y, x, y], axis=1), np.full(n, 10000.0), rcond=None)[0]
    cx, cy = np.linalg.solve(np.array([[2 * g[0], g[2]], [g[2], 2 * g[1]]]), g[3:5])
    dx, dy = x - cx, y - cy
    f = np.linalg.lstsq(np.stack([dx * dx, dy * dy, dx * dy], axis=1), np.ones(n), rcond=None)[0]
    lam = np.linalg.eigvalsh(np.array([[f[0], 0.5 * f[2]], [0.5 * f[2], f[1]]]))
    if not lam[0] > 0:
        raise IllPosed(f"the fitted conic is no ellipse (eigenvalues {lam})")
    long_, short = 2.0 / math.sqrt(lam[0]) / k, 2.0 / math.sqrt(lam[1]) / k
    return short * um, long_ * um, math.sqrt(1.0 - (short / long_) ** 2)


def ref_closed_form(area: float, perimeter: float, um: float = UM) -> dict:
    """CircularED, Circularity, Chords, Sphericity (index into the 12 -> value); the product scales each by um_pix."""
    if perimeter == 0:
        return {5: math.sqrt(4 * area / math.pi) * um, 7: 0.0, 8: 0.0, 11: 0.0}
    return {5: math.sqrt(4 * area / math.pi) * um, 7: 4 * math.pi * area / perimeter ** 2 * um, 8: perimeter * um,
            11: 2 * math.sqrt(math.pi * area) / perimeter * um}


def ellipse_bound(n: int) -> float:
    return ELLIPSE_BOUND_SMALL_N if n < 10 else ELLIPSE_BOUND


def check_against_reference(values: Sequence[float], points: np.ndarray, area: float, perimeter: float, um: float = UM,
                            ellipse: bool = True, rel: float = 0.0, ties: str = "raise") -> List[str]:
    """Everything wrong with the 12 ``values`` of one contour, judged by the float64 reference alone (``rel``: see
    :func:`match_rect`, ``ties``: see :func:`min_area_rectangles`; ``ellipse=False`` leaves out the three ellipse values of a contour of five or more points)."""
    bad = []
    r = match_rect(values, points, um, rel, ties)
    if r:
        bad.append(r)
    for j, e in ref_closed_form(area, perimeter, um).items():
        if abs(values[j] - e) > CLOSED_TOL * abs(e):
            bad.append(f"{KEYS[j]} {values[j]!r} != closed form {e!r}")
    if len(points) < 5:
        if any(values[j] != 0 for j in ELLIPSE_IDX):
            bad.append(f"ellipse values of {len(points)} points must be 0: {[values[j] for j in ELLIPSE_IDX]}")
    elif ellipse:
        for j, e in zip(ELLIPSE_IDX, ref_ellipse(points, um)):
            if abs(values[j] - e) > ellipse_bound(len(points)) * abs(e):
                bad.append(f"{KEYS[j]} {values[j]!r} != {e!r} (rel {abs(values[j] - e) / abs(e):.3g})")
    return bad


def oracle_values(points: np.ndarray, um: float = UM) -> Tuple[np.ndarray, bool]:
    """The CPU oracle's 12 values and its flag for a rounding-dependent ellipse fit."""
    from oracle import postproc_ref as P

    r = P.calculate_measurements(np.asarray(points, dtype=np.int32), um_pix=um)
    return np.array([float(r[k]) for k in KEYS]), bool(r["_ellipse_unstable"])


# ----------------------------------------------------------------------------------------------------------------------
# the tables demia_contour_measure reads
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Tables:
    M: int
    C: int
    max_points: int
    count: "object"      # int32 [M]
    info: "object"       # int32 [M, C, 4]: start x, start y, n, off
    red: "object"        # float64 [M, C, 2]: area, perimeter
    points: "object"     # int32 [max_points, 2]
    host_info: np.ndarray
    host_red: np.ndarray


SPARE = 4                # the tracer's contract: contour t owns [off, off + n + SPARE) of the point pool
POOL_FILL = -12345       # what every unowned and spare slot of the pool holds


def tables_from_points(contours_per_mask: Sequence[Sequence[np.ndarray]], C: int, device, pool_order: Optional[Sequence[int]] = None,
                       gap: int = 0, lead: int = 0) -> Tables:
    """Tables as the tracer would leave them for the given integer point lists: contour c of mask m in slot (m, c); area and
    perimeter from the oracle's contourArea / arcLength.  ``pool_order`` permutes the order in which the contours (numbered
    mask by mask) are laid into the point pool, ``lead`` slots stay free in front and ``gap`` between two contours."""
    import torch

    from oracle import postproc_ref as P

    M = len(contours_per_mask)
    flat = [(m, c, np.asarray(pts, dtype=np.int32).reshape(-1, 2)) for m, cs in enumerate(contours_per_mask) for c, pts in enumerate(cs)]
    assert all(len(cs) <= C for cs in contours_per_mask)
    order = list(range(len(flat))) if pool_order is None else list(pool_order)
    assert sorted(order) == list(range(len(flat)))
    max_points = lead + sum(len(p) + SPARE + gap for _, _, p in flat) + 7
    count = np.array([len(cs) for cs in contours_per_mask], dtype=np.int32)
    info = np.zeros((M, C, 4), dtype=np.int32)
    red = np.zeros((M, C, 2), dtype=np.float64)
    pool = np.full((max_points, 2), POOL_FILL, dtype=np.int32)
    off = lead
    for t in order:
        m, c, pts = flat[t]
        n = len(pts)
        assert n >= 1 and off + n + SPARE <= max_points
        pool[off: off + n] = pts
        info[m, c] = (pts[0, 0], pts[0, 1], n, off)
        red[m, c] = (P.contour_area(pts), P.arc_length(pts))
        off += n + SPARE + gap
    dev = torch.device(device)
    return Tables(M, C, max_points, torch.from_numpy(count).to(dev), torch.from_numpy(info).to(dev), torch.from_numpy(red).to(dev),
                  torch.from_numpy(pool).to(dev), info, red)


OUT_FILL = -7.25         # what measure_tables() fills the output with before the launch
OUT_GUARD = 6 * 12       # doubles behind the output that must still hold OUT_FILL after it


def measure_tables(t: Tables, um: float = UM, select: Optional[Sequence[int]] = None, out_c: Optional[int] = None) -> np.ndarray:
    """One launch of ``demia_contour_measure`` over the tables: [M, out_c, 12] float64, rows the kernel did not write hold
    ``OUT_FILL``.  ``select``: the masks to measure (default all); ``out_c``: contour slots per mask in the output (default C).
    Asserts that nothing was written behind the last row."""
    import torch

    from deepemia_amd import _lib

    lib = _lib.load()
    dev = t.count.device
    out_c = t.C if out_c is None else int(out_c)
    sel = None
    if select is not None:
        flags = np.zeros(t.M, dtype=np.int32)
        flags[np.asarray(list(select), dtype=np.int64)] = 1
        sel = torch.from_numpy(flags).to(dev)
    wi = torch.empty((int(lib.demia_contour_work_ints(t.M, t.C, t.max_points)),), dtype=torch.int32, device=dev)
    wf = torch.empty((int(lib.demia_contour_work_floats(t.M, t.C, t.max_points)),), dtype=torch.float32, device=dev)
    wd = torch.empty((int(lib.demia_contour_work_doubles(t.M, t.C, t.max_points)),), dtype=torch.float64, device=dev)
    flat = torch.full((t.M * out_c * 12 + OUT_GUARD,), OUT_FILL, dtype=torch.float64, device=dev)
    out = flat[: t.M * out_c * 12].view(t.M, out_c, 12)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.demia_contour_measure(_lib.ptr(sel), _lib.ptr(t.count), _lib.ptr(t.info), _lib.ptr(t.red), _lib.ptr(t.points),
                                             t.M, t.C, t.max_points, _lib.ptr(wi), _lib.ptr(wf), _lib.ptr(wd), float(um),
                                             _lib.ptr(out), out_c, stream), "demia_contour_measure")
        host = flat.cpu().numpy()
    assert (host[t.M * out_c * 12:] == OUT_FILL).all(), "demia_contour_measure wrote behind its output"
    return host[: t.M * out_c * 12].reshape(t.M, out_c, 12)


# ----------------------------------------------------------------------------------------------------------------------
# degenerate contours with known answers
# ----------------------------------------------------------------------------------------------------------------------
def degenerate_cases() -> List[Case]:
    """Fed to the kernel as they are (no tracer would produce most of them)."""
    i = np.array([3, 0, 5, 1, 4, 2])
    return [Case("one_point", np.array([[700, 900]], dtype=np.int32)),
            Case("two_horizontal", np.array([[1200, 345], [1290, 345]], dtype=np.int32)),
            Case("triangle", np.array([[100, 100], [180, 130], [120, 220]], dtype=np.int32)),
            Case("rectangle", np.array([[3005, 7], [3005, 26], [3014, 26], [3014, 7]], dtype=np.int32)),
            Case("collinear6", np.stack([2000 + 7 * i, 40 + 7 * i], axis=1).astype(np.int32)),
            Case("identical5", np.full((5, 2), 4321, dtype=np.int32))]


def two_point_closed_form(p0, p1, um: float = UM) -> Tuple[float, float]:
    """(Length, Width) of a hull of two integer points: a rectangle of zero height, whose corners are the two ends."""
    return 0.0, math.hypot(p1[0] - p0[0], p1[1] - p0[1]) * um
