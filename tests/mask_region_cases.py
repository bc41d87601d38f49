"""What ``test_cpu_mask_region_cases.py`` and ``test_gpu_mask_region_edges.py`` share: the case table for the per-mask REGION
stages of ``csrc/maskregion.h`` (flood by band sweeps, ``outside_background`` / ``fill_holes`` / ``has_holes``, the Euler
shortcut and ``more_than_one_component``, ``morph_cross``) as ``run_mask_program`` (``csrc/maskops.hip``) drives them, and a
numpy restatement of the kernel's STRUCTURE -- not of its arithmetic -- that the CPU test uses to show that every case sits
where its name says and that the scipy-backed reference (``oracle/postproc_ref.py``) can tell a structurally wrong flood
from a right one.

Restated from the kernel (the CPU test pins each of them against the cases):

* ``region_of``: the hint box grown by ``e = dilations + 1`` pixels, clipped to the frame, in rows x 32-pixel word columns;
* the variant rule on ``n = rh * rw`` words: ``n <= 1024`` small LDS variant (256 threads = 4 waves), ``n <= 8192`` large LDS
  variant (512 threads = 8 waves), above that the same 512 threads on the planes in HBM;
* the flood's two bodies: ``rw <= 64`` one lane per word ("lane"), wider regions in 64-word chunks ("chunk");
* the band partition ``rpb = ceil(rh / nw)`` rows per wave (waves beyond ``ceil(rh / rpb)`` own nothing);
* the seeds of ``outside_background`` and the flood's round limit ``2 * (rh + 32 * rw) + 8`` as it stood when these tests were
  written (``legacy_max_rounds``) beside the proven one (``proven_max_rounds``).

The LOCKSTEP model (:func:`lockstep_flood`) is the schedule in which all waves run in step: every round each band sweeps down
and then up, a row's in-row propagation is complete, and the row a sweep reads from the neighbouring band is the one that
band had at the START of the sweep.  It works on horizontal runs (a run is filled as a whole) and gives every run the
(round, sweep) in which it is filled by a shortest-path pass with waiting edges, so a 130 x 2040 serpentine costs a second,
not the minutes a pixel simulation of 8000 rounds would.  Real waves drift, so hardware may need fewer or more rounds than
this; what the model shows is that the number of rounds is not bounded by the region's perimeter.

Nothing in here needs a GPU.
"""
from __future__ import annotations

import heapq
from dataclasses import dataclass, replace
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

SMALL_WORDS = 1024            # REG_WORDS_SMALL
LARGE_WORDS = 8192            # REG_WORDS
LANE_WORDS = 64               # widest region of the register-carried flood body
HINTS = ("tight", "loose", "frame")
LOOSE = (7, 40)               # rows, columns a loose hint adds on every side (clipped to the frame)

Box = Tuple[int, int, int, int]            # y0, x0, y1, x1 inclusive; (-1, -1, -1, -1): empty
EMPTY: Box = (-1, -1, -1, -1)


# ----------------------------------------------------------------------------------------------------------------------
# the kernel's rules, restated
# ----------------------------------------------------------------------------------------------------------------------
def n_dilations(program: Sequence[str]) -> int:
    return sum(1 for s in program if s == "dilate")


def region_of(box: Box, e: int, H: int, W: int) -> Tuple[int, int, int, int]:
    """(ry0, wx0, rh, rw) of mreg::region_of."""
    y0, x0, y1, x1 = box
    ry0 = max(y0 - e, 0)
    ry1 = min(y1 + e, H - 1)
    wx0 = max(x0 - e, 0) >> 5
    wx1 = min(x1 + e, W - 1) >> 5
    return ry0, wx0, ry1 - ry0 + 1, wx1 - wx0 + 1


def variant(n: int) -> str:
    return "small" if n <= SMALL_WORDS else ("large" if n <= LARGE_WORDS else "hbm")


def waves(n: int) -> int:
    return 4 if n <= SMALL_WORDS else 8


def legacy_max_rounds(rh: int, rw: int) -> int:
    return 2 * (rh + 32 * rw) + 8


def proven_max_rounds(rh: int, rw: int) -> int:
    """Every round but the last sets at least one of the region's 32 * rh * rw bits."""
    return 32 * rh * rw + 1


def tight_box(mask: np.ndarray) -> Box:
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return EMPTY
    return int(ys.min()), int(xs.min()), int(ys.max()), int(xs.max())


def hint_box(mask: np.ndarray, kind: str) -> Box:
    H, W = mask.shape
    t = tight_box(mask)
    if t == EMPTY or kind == "tight":
        return t
    if kind == "frame":
        return 0, 0, H - 1, W - 1
    assert kind == "loose"
    return max(t[0] - LOOSE[0], 0), max(t[1] - LOOSE[1], 0), min(t[2] + LOOSE[0], H - 1), min(t[3] + LOOSE[1], W - 1)


def box_for_region(ry0: int, wx0: int, rh: int, rw: int, e: int) -> Box:
    """The tight box whose region (grown by e, not clipped) is exactly rows ry0 .. ry0+rh-1, words wx0 .. wx0+rw-1."""
    assert rh > 2 * e and ry0 >= 0 and wx0 >= 0
    return ry0 + e, wx0 * 32 + e, ry0 + rh - 1 - e, (wx0 + rw) * 32 - 1 - e


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    family: str
    mask: np.ndarray                       # (H, W) bool
    program: Tuple[str, ...]
    hint: str = "tight"
    claim: Tuple[Tuple[str, object], ...] = ()      # geometry the name promises, for `hint` and `program`
    active: Optional[int] = None           # F: the gate's byte (None: no `active` array at all)

    @property
    def H(self) -> int:
        return int(self.mask.shape[0])

    @property
    def W(self) -> int:
        return int(self.mask.shape[1])


def geometry(c: Case, hint: Optional[str] = None) -> Dict[str, object]:
    """Where the kernel puts this case: region, variant, flood body, band partition."""
    box = hint_box(c.mask, hint or c.hint)
    if box == EMPTY:
        return {"empty": True}
    e = n_dilations(c.program) + 1
    ry0, wx0, rh, rw = region_of(box, e, c.H, c.W)
    n = rh * rw
    nw = waves(n)
    rpb = -(-rh // nw)
    return {"empty": False, "box": box, "e": e, "ry0": ry0, "wx0": wx0, "rh": rh, "rw": rw, "n": n, "variant": variant(n), "nw": nw,
            "rpb": rpb, "bands": -(-rh // rpb), "body": "lane" if rw <= LANE_WORDS else "chunk",
            "clipped": (box[0] - e < 0, box[1] - e < 0, box[2] + e > c.H - 1, box[3] + e > c.W - 1)}


def run_program_ref(mask: np.ndarray, program: Sequence[str], active: Optional[int], P) -> Tuple[np.ndarray, int]:
    """The stage program on a dense mask with the oracle's scipy-backed stages (P = oracle.postproc_ref): (mask, flag)."""
    m = mask.astype(bool).copy()
    flag = 0
    for op in program:
        if op == "fill":
            m = P.fill_holes(m)
        elif op == "dilate":
            m = P.dilate_cross(m)
        elif op == "erode":
            m = P.erode_cross(m)
        elif op in ("drop_multi", "flag_multi"):
            multi = P.n_components8(m) > 1
            flag |= int(multi)
            if multi and op == "drop_multi":
                m = np.zeros_like(m)
        elif op == "gate":
            if not active:
                break
        else:
            raise ValueError(op)
    return m, flag


def _pin(m: np.ndarray, box: Box) -> None:
    m[box[0], box[1]] = True
    m[box[2], box[3]] = True


def _ring(m: np.ndarray, y0: int, x0: int, y1: int, x1: int) -> None:
    """1-px rectangle outline (encloses its interior when it is at least 3 x 3)."""
    m[y0, x0:x1 + 1] = True
    m[y1, x0:x1 + 1] = True
    m[y0:y1 + 1, x0] = True
    m[y0:y1 + 1, x1] = True


def _channel_cavity(m: np.ndarray, ya: int, yb: int, x_cav0: int, x_cav1: int, x_open: int) -> None:
    """A walled cavity (columns x_cav0 .. x_cav1 inside rows ya .. yb) whose only way out is a 1-px horizontal channel in row
    (ya + yb) // 2, walled above and below, that ends open at column x_open (right of the cavity if x_open > x_cav1, else left)."""
    yc = (ya + yb) // 2
    m[ya:yb + 1, x_cav0 - 1:x_cav1 + 2] = True
    lo, hi = (x_cav1 + 1, x_open) if x_open > x_cav1 else (x_open, x_cav0 - 1)
    m[yc - 1:yc + 2, lo:hi + 1] = True
    m[ya + 1:yb, x_cav0:x_cav1 + 1] = False
    m[yc, lo:hi + 1] = False


def _ring_and_cups(H: int, W: int, box: Box) -> np.ndarray:
    """Pinned to `box`: a ring with an island in its hole, a cup open to the top, one open to the bottom, a cup open to the left."""
    m = np.zeros((H, W), dtype=bool)
    y0, x0, y1, x1 = box
    _pin(m, box)
    ym = (y0 + y1) // 2
    xa, xb = x0 + 3, x0 + (x1 - x0) // 3
    _ring(m, y0 + 2, xa, y1 - 2, xb)
    m[ym - 1:ym + 2, (xa + xb) // 2 - 1:(xa + xb) // 2 + 2] = True
    xc, xd = xb + 4, x0 + 2 * (x1 - x0) // 3
    _ring(m, y0 + 2, xc, ym - 2, xd)
    m[y0 + 2, (xc + xd) // 2] = False                                  # open to the top
    _ring(m, ym + 2, xc, y1 - 2, xd)
    m[y1 - 2, (xc + xd) // 2 + 1] = False                              # open to the bottom
    _ring(m, y0 + 2, xd + 4, y1 - 2, x1 - 3)
    m[ym, xd + 4] = False                                              # open to the left
    return m


# ---- A: variant boundaries ----------------------------------------------------------------------------------------------
A_FRAME = (140, 2144)
A_SIZES = ((32, 32, "small"), (33, 32, "large"), (128, 64, "large"), (129, 64, "hbm"))
A_PROGRAMS = (("fill",), ("fill", "dilate", "erode"))


def family_a() -> List[Case]:
    out = []
    H, W = A_FRAME
    for rh, rw, cls in A_SIZES:
        for prog in A_PROGRAMS:
            e = n_dilations(prog) + 1
            box = box_for_region(3, 1, rh, rw, e)
            out.append(Case(f"A_{rh}x{rw}_{cls}_{'+'.join(prog)}", "A", _ring_and_cups(H, W, box), prog,
                            claim=(("rh", rh), ("rw", rw), ("variant", cls), ("wx0", 1), ("body", "lane"))))
    return out


def mixed_batch() -> Tuple[List[Case], Tuple[str, ...]]:
    """One batch with all three classes and an empty mask, for the two C entries (worklist / plain)."""
    prog = ("fill", "dilate", "erode")
    cs = [c for c in family_a() if c.program == prog and c.claim[0][1] in (32, 33, 129)]
    cs.append(Case("A_empty", "A", np.zeros(A_FRAME, dtype=bool), prog))
    return cs, prog


# ---- B: regions wider than 64 words -------------------------------------------------------------------------------------
B_FRAME = (140, 4288)
B_WX0 = 3
B_WIDTHS = (65, 66, 129, 130)


def _b_fill_mask(box: Box, bounds: Sequence[int]) -> np.ndarray:
    """Across every chunk boundary xb (first pixel column of region word 64 / 128): a hole that straddles it, a cavity left of
    it whose channel opens right of it (the front crosses right to left), and the mirror image."""
    m = np.zeros(B_FRAME, dtype=bool)
    _pin(m, box)
    y = box[0]
    for xb in bounds:
        _ring(m, y + 2, xb - 5, y + 8, xb + 5)
        _channel_cavity(m, y + 11, y + 19, xb - 24, xb - 12, xb + 10)
        _channel_cavity(m, y + 22, y + 30, xb + 12, xb + 24, xb - 10)
    return m


def _b_diag_mask(box: Box, bounds: Sequence[int], left_row: int, right_row: int, spine_right: bool, spine_top: int) -> np.ndarray:
    """Two bars that meet only diagonally across the LAST chunk boundary (and run straight across any earlier one), a spine
    down one side that carries a small ring (the hole that forces the 8-connected flood), one component in all."""
    m = np.zeros(B_FRAME, dtype=bool)
    y0, x0, y1, x1 = box
    xb = bounds[-1]
    m[y0 + left_row, x0:xb] = True
    m[y0 + right_row, xb:x1 + 1] = True
    xs = x1 if spine_right else x0
    m[y0 + spine_top:y1 + 1, xs] = True
    xr = xs - 2 if spine_right else xs
    _ring(m, y0 + 5, xr, y0 + 7, xr + 2)
    return m


# name (bs: the link runs down to the right, sl: up to the right; where the raster-first pixel lies), rows of the left and the
# right bar, spine on the right, first row of the spine
B_DIAG = (("bs_first_left", 0, 1, False, 0), ("sl_first_right", 1, 0, False, 1), ("sl_first_left", 2, 1, False, 0),
          ("bs_first_right", 1, 2, True, 0))


def family_b() -> List[Case]:
    out = []
    for rw in B_WIDTHS:
        for cls, rh in (("large", LARGE_WORDS // rw), ("hbm", LARGE_WORDS // rw + 1)):
            box = box_for_region(2, B_WX0, rh, rw, 1)
            bounds = [(B_WX0 + k) * 32 for k in (64, 128) if k < rw]
            claim = (("rh", rh), ("rw", rw), ("variant", cls), ("wx0", B_WX0), ("body", "chunk"))
            fm = _b_fill_mask(box, bounds)
            out.append(Case(f"B_rw{rw}_{cls}_holes+channels_fill", "B", fm, ("fill",), claim=claim))
            out.append(Case(f"B_rw{rw}_{cls}_holes+channels_multi", "B", fm, ("flag_multi",), claim=claim))
            for name, lr, rr, sr, st in B_DIAG:
                dm = _b_diag_mask(box, bounds, lr, rr, sr, st)
                out.append(Case(f"B_rw{rw}_{cls}_diag_{name}_multi", "B", dm, ("flag_multi",), claim=claim))
                if name == "bs_first_left":
                    out.append(Case(f"B_rw{rw}_{cls}_diag_{name}_fill", "B", dm, ("fill",), claim=claim))
    return out


# ---- C: bands -----------------------------------------------------------------------------------------------------------
C_ROWS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17)
C_W = 11040                                                    # 345 words: room for rw = 1024 // 3 + 1 = 342
C_PROGRAMS = (("fill",), ("flag_multi",))


def _c_content(H: int, W: int, box: Box) -> np.ndarray:
    """Pinned to `box`; at its left end, across a word boundary in its middle and at its right end: a ring as high as the box,
    a 1-px vertical channel open at the top and one open at the bottom -- each crosses every band of the region."""
    m = np.zeros((H, W), dtype=bool)
    y0, x0, y1, x1 = box
    _pin(m, box)
    hb = y1 - y0 + 1
    for c in (x0 + 2, ((x0 + x1) // 2) // 32 * 32 - 9, x1 - 19):
        if hb >= 3:
            _ring(m, y0, c, y1, c + 4)
        else:
            m[y0:y1 + 1, c] = True; m[y0:y1 + 1, c + 2] = True; m[y0, c + 4] = True           # noqa: E702
        if hb >= 2:
            m[y0:y1 + 1, c + 8:c + 11] = True
            m[y0:y1, c + 9] = False                                # open at the top
            m[y0:y1 + 1, c + 14:c + 17] = True
            m[y0 + 1:y1 + 1, c + 15] = False                       # open at the bottom
        else:
            m[y0, c + 8] = True; m[y0, c + 10:c + 12] = True        # noqa: E702
    return m


def family_c() -> List[Case]:
    out = []
    for rh in C_ROWS:
        shapes = [("w4", 3)] + ([("w8", SMALL_WORDS // rh + 1)] if rh >= 3 else [])
        for tag, rw in shapes:
            if rh <= 2:                                            # the frame is the region's height: rows 0 and H - 1 coincide or touch
                H = rh
                box = (0, 33, rh - 1, (1 + rw) * 32 - 2)
            else:
                H = 24
                box = box_for_region(2, 1, rh, rw, 1)
            m = _c_content(H, C_W, box)
            n = rh * rw
            for prog in C_PROGRAMS:
                out.append(Case(f"C_rh{rh}_{tag}_{prog[0]}", "C", m, prog,
                                claim=(("rh", rh), ("rw", rw), ("nw", 4 if tag == "w4" else 8), ("variant", variant(n)), ("wx0", 1))))
    return out


# ---- D: frame edges -----------------------------------------------------------------------------------------------------
D_WIDTHS = (1, 31, 32, 33, 63, 64, 65)
D_HEIGHTS = (1, 2, 3, 40)
D_PROGRAMS = (("fill",), ("erode",), ("dilate",), ("dilate", "erode"), ("flag_multi",))


def _d_masks(H: int, W: int) -> List[Tuple[str, np.ndarray]]:
    full = np.ones((H, W), dtype=bool)
    border = np.zeros((H, W), dtype=bool)
    _ring(border, 0, 0, H - 1, W - 1)
    inner = np.zeros((H, W), dtype=bool)
    if H >= 3 and W >= 3:
        _ring(inner, 1, 1, H - 2, W - 2)
    corners = np.zeros((H, W), dtype=bool)
    corners[0, 0] = corners[0, W - 1] = corners[H - 1, 0] = corners[H - 1, W - 1] = True
    cav = np.zeros((H, W), dtype=bool)                             # cavities open only to a frame edge: never filled
    r = min(2, H - 1)
    cav[0:r + 1, max(W - 4, 0):] = True
    cav[min(1, r), max(W - 3, 0):] = False                         # open to the right edge (pixel W - 1)
    if H >= 8 and W >= 8:
        cav[H - 3:, 0:4] = True
        cav[H - 2, 0:3] = False                                    # open to the left edge
        cav[H - 4:, W // 2 - 1:W // 2 + 2] = True
        cav[H - 3:, W // 2] = False                                # open to the bottom edge
        cav[0:4, W // 2 - 1:W // 2 + 2] = True
        cav[0:3, W // 2] = False                                   # open to the top edge
        cav[10:15, W - 6:W - 1] = True                             # ... and one closed cavity one pixel inside the right edge: filled
        cav[11:14, W - 5:W - 2] = False
    return [("full", full), ("border", border), ("ring_inside_border", inner), ("corners", corners), ("edge_cavities", cav)]


def family_d() -> List[Case]:
    out = []
    for W in D_WIDTHS:
        for H in D_HEIGHTS:
            for name, m in _d_masks(H, W):
                for prog in D_PROGRAMS:
                    out.append(Case(f"D_{H}x{W}_{name}_{'+'.join(prog)}", "D", m, prog, claim=(("variant", "small"),)))
    return out


# ---- F: programs --------------------------------------------------------------------------------------------------------
F_FRAME = (50, 77)
F_PROGRAMS = ((("dilate",) * 4 + ("erode",) * 4, None), (("fill", "dilate", "dilate", "erode", "erode"), None),
              (("flag_multi", "dilate", "flag_multi"), None), (("drop_multi", "fill", "dilate"), None),
              (("gate", "dilate"), None), (("gate", "dilate"), 0), (("gate", "dilate"), 1))


def _f_masks() -> List[Tuple[str, np.ndarray]]:
    H, W = F_FRAME
    out = []
    for corner in ("br", "tl"):
        two = np.zeros((H, W), dtype=bool)
        two[H - 7:H - 1, W - 11:W - 7] = True
        two[H - 7:H - 1, W - 5:W - 1] = True                       # 2 px apart: one dilation joins them
        one = np.zeros((H, W), dtype=bool)
        one[H - 9:H - 1, W - 10:W - 1] = True
        one[H - 6, W - 14:W - 10] = True
        ring = np.zeros((H, W), dtype=bool)
        _ring(ring, H - 12, W - 13, H - 2, W - 2)
        ring[H - 8:H - 6, W - 9:W - 7] = True                      # an island in the hole
        for name, m in (("two_2px_apart", two), ("one", one), ("ring_with_island", ring)):
            out.append((f"{name}_{corner}", m if corner == "br" else m[::-1, ::-1].copy()))
    return out


def family_f() -> List[Case]:
    out = []
    for prog, active in F_PROGRAMS:
        for name, m in _f_masks():
            out.append(Case(f"F_{'+'.join(prog)}_active{active}_{name}", "F", m, prog, active=active))
    return out


# ---- G: component count -------------------------------------------------------------------------------------------------
G_FRAME = (48, 100)


def _g_masks() -> List[Tuple[str, str, np.ndarray]]:
    H, W = G_FRAME

    def z():
        return np.zeros((H, W), dtype=bool)

    out = []
    m = z(); m[20, 63] = True; out.append(("one_pixel", "euler", m))                                            # noqa: E702
    m = z(); m[np.arange(10, 30), np.arange(54, 74)] = True; out.append(("diagonal_chain", "euler", m))          # noqa: E702
    m = z()                                                                                                        # 2x2 blocks, corners touching
    for k in range(6):
        m[10 + 2 * k:12 + 2 * k, 56 + 2 * k:58 + 2 * k] = True
    out.append(("checker_blocks", "euler", m))
    m = z(); m[10:20, 50:64] = True; m[20:30, 64:80] = True; out.append(("blobs_touch_at_corner", "euler", m))   # noqa: E702
    m = z(); m[10:20, 50:63] = True; m[10:20, 64:80] = True; out.append(("blobs_1px_apart", "euler", m))         # noqa: E702
    m = z(); m[10, 40:90] = True; m[10:40, 40:90:2] = True; out.append(("comb", "euler", m))                     # noqa: E702
    m = z(); _ring(m, 8, 40, 40, 90); out.append(("ring", "flood", m))                                           # noqa: E702
    m = z(); _ring(m, 8, 40, 40, 90); m[20:24, 62:66] = True; out.append(("ring_island_inside", "flood", m))     # noqa: E702
    m = z(); _ring(m, 8, 40, 40, 90); m[20:24, 94:97] = True; out.append(("ring_island_outside", "flood", m))    # noqa: E702
    m = z(); _ring(m, 8, 40, 20, 64); _ring(m, 21, 65, 40, 90); out.append(("rings_touch_diagonally", "flood", m))   # noqa: E702
    m = z(); _ring(m, 8, 40, 40, 90); m[6, 38] = True; out.append(("speck_first_then_ring", "flood", m))         # noqa: E702
    return out


def family_g() -> List[Case]:
    out = []
    for name, path, m in _g_masks():
        for prog in (("flag_multi",), ("fill",)):
            out.append(Case(f"G_{path}_{name}_{prog[0]}", "G", m, prog, claim=(("path", path),)))
    return out


# ---- H: the flood's round limit -----------------------------------------------------------------------------------------
H_FRAME = (140, 2200)
H_PROGRAMS = (("fill",), ("flag_multi",))


def serpentine(h: int, w: int, vertical: bool = True) -> np.ndarray:
    """h x w box of 1-px walls around one 1-px channel, pitch 2, that winds through the whole box from its single opening (top
    left) to a dead end: one component, no hole, and a background path about h * w / 2 pixels long."""
    if not vertical:
        return serpentine(w, h, True).T.copy()
    m = np.zeros((h, w), dtype=bool)
    m[0, :] = True
    m[h - 1, :] = True
    m[:, 0:w:2] = True
    m[:, w - 1] = True
    for k, c in enumerate(range(2, w - 2, 2)):                     # inner walls: a gap at the bottom, then at the top, ...
        m[h - 2 if k % 2 == 0 else 1, c] = False
    m[0, 1] = False                                                # the opening
    return m


# name, box height, box width, vertical legs, first pixel column, adversarial for 8 waves
H_SIZES = (("64x500_lds8", 64, 500, True, 33, True), ("130x2040_hbm", 130, 2040, True, 33, True),
           ("20x2080_chunk", 20, 2080, True, 33, True), ("30x250_control", 30, 250, True, 33, False),
           ("64x500_horizontal", 64, 500, False, 33, False))
H_CLAIMS = {"64x500_lds8": (("rh", 66), ("rw", 16), ("variant", "large"), ("nw", 8), ("body", "lane")),
            "130x2040_hbm": (("rh", 132), ("rw", 64), ("variant", "hbm"), ("nw", 8), ("body", "lane")),
            "20x2080_chunk": (("rh", 22), ("rw", 66), ("variant", "large"), ("nw", 8), ("body", "chunk"), ("wx0", 1)),
            "30x250_control": (("rh", 32), ("rw", 8), ("variant", "small"), ("nw", 4), ("body", "lane")),
            "64x500_horizontal": (("rh", 66), ("rw", 16), ("variant", "large"), ("nw", 8), ("body", "lane"))}


def family_h() -> List[Case]:
    out = []
    for name, h, w, vert, x0, _ in H_SIZES:
        m = np.zeros(H_FRAME, dtype=bool)
        m[3:3 + h, x0:x0 + w] = serpentine(h, w, vert)
        for prog in H_PROGRAMS:
            out.append(Case(f"H_{name}_{prog[0]}", "H", m, prog, claim=H_CLAIMS[name]))
    return out


FAMILIES = {"A": family_a, "B": family_b, "C": family_c, "D": family_d, "F": family_f, "G": family_g, "H": family_h}
_CACHE: Dict[str, List[Case]] = {}


def cases(family: str) -> List[Case]:
    if family not in _CACHE:
        _CACHE[family] = FAMILIES[family]()
        names = [c.name for c in _CACHE[family]]
        assert len(set(names)) == len(names), family
    return _CACHE[family]


def with_hint(c: Case, hint: str) -> Case:
    return replace(c, hint=hint)


def batches(cs: Sequence[Case]) -> List[List[Case]]:
    """Cases that share frame, program and gate go through one call."""
    groups: Dict[tuple, List[Case]] = {}
    for c in cs:
        groups.setdefault((c.H, c.W, c.program, c.active), []).append(c)
    return list(groups.values())


# ----------------------------------------------------------------------------------------------------------------------
# the lockstep model of mreg::flood
# ----------------------------------------------------------------------------------------------------------------------
def lockstep_flood(passm: np.ndarray, seed: np.ndarray, rpb: int, eight: bool, limit: Optional[int] = None, split_cols: Sequence[int] = (),
                   band_links: bool = True, diag_across_words: bool = True) -> Tuple[np.ndarray, int]:
    """``flood<eight>`` on an rh x (32 rw) pixel region with all waves in step.  passm: where the front may go; seed: the bits of R
    on entry (a subset of passm).  Returns (R at the end, number of rounds in which some word changed); ``limit``: R after that
    many rounds.  A flood is complete under a round limit L iff the returned count is <= L.

    Deliberate faults, for the CPU test: ``split_cols`` (no link of any kind across these pixel columns), ``band_links=False``
    (no link between the bands of two waves), ``diag_across_words=False`` (no diagonal link across a 32-pixel word boundary)."""
    h, w = passm.shape
    seed = seed & passm
    start = passm.copy()
    start[:, 1:] &= ~passm[:, :-1]
    for c in split_cols:
        start[:, c] = passm[:, c]
    nr = int(start.sum())
    if nr == 0:
        return np.zeros_like(passm), 0
    rid = np.cumsum(start.ravel()).reshape(h, w) - 1
    rid[~passm] = -1
    row_of = np.repeat(np.arange(h), start.sum(1)).tolist()
    # links between row y - 1 (upper) and row y (lower): slices of the two rows, and which links survive the faults
    lower_rows = np.arange(1, h)
    row_keep = np.ones(h - 1, dtype=bool) if band_links else (lower_rows % rpb != 0)
    band_first = lower_rows % rpb == 0
    cross = np.arange(1, w)                                        # a diagonal link between columns x and x + 1 crosses column x + 1
    diag_keep = np.ones(w - 1, dtype=bool)
    diag_keep[np.asarray([c - 1 for c in split_cols if 0 < c < w], dtype=np.int64)] = False
    if not diag_across_words:
        diag_keep[cross % 32 == 0] = False
    combos = [(np.s_[:-1, :], np.s_[1:, :], None)]
    if eight:
        combos += [(np.s_[:-1, :-1], np.s_[1:, 1:], diag_keep), (np.s_[:-1, 1:], np.s_[1:, :-1], diag_keep)]
    keys, t0 = [], [rid[seed]]
    for us, ls, ck in combos:
        a, b = rid[us], rid[ls]
        ok = (a >= 0) & (b >= 0) & row_keep[:, None]
        raw = seed[us] & passm[ls] & (band_first & row_keep)[:, None]      # round 0: a band's first row sees the raw seed bits above it
        if ck is not None:
            ok &= ck[None, :]
            raw &= ck[None, :]
        keys.append(a[ok].astype(np.int64) * nr + b[ok])
        t0.append(b[raw])
    keys = np.unique(np.concatenate(keys))
    up_of, lo_of = keys // nr, keys % nr                           # sorted by upper run

    def csr(src, dst):
        o = np.argsort(src, kind="stable")
        ptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=nr))])
        return ptr.tolist(), dst[o].tolist()

    dptr, didx = csr(up_of, lo_of)                                 # run -> the runs below it
    uptr, uidx = csr(lo_of, up_of)                                 # run -> the runs above it
    INF = 1 << 60
    t = [INF] * nr                                                 # phase in which the run is filled: 2 * round + (0 down sweep, 1 up sweep)
    heap = []
    for r in np.unique(np.concatenate(t0)).tolist():
        t[r] = 0
        heap.append((0, r))
    heapq.heapify(heap)
    while heap:
        tt, r = heapq.heappop(heap)
        if tt > t[r]:
            continue
        y = row_of[r]
        # downwards: filled by the next down sweep (even phase) that sees this run -- the same sweep inside a band, a LATER one
        # across a band boundary (the neighbour's row is read when the sweep starts)
        base = tt + 1 if (y + 1) % rpb == 0 else tt
        t2 = base + (base & 1)
        for k in range(dptr[r], dptr[r + 1]):
            q = didx[k]
            if t2 < t[q]:
                t[q] = t2
                heapq.heappush(heap, (t2, q))
        base = tt + 1 if y % rpb == 0 else tt
        t2 = base + 1 - (base & 1)
        for k in range(uptr[r], uptr[r + 1]):
            q = uidx[k]
            if t2 < t[q]:
                t[q] = t2
                heapq.heappush(heap, (t2, q))
    ta = np.asarray(t, dtype=np.int64)
    reached = ta < INF
    rounds = int(ta[reached].max() // 2 + 1) if reached.any() else 0
    if limit is not None:
        reached &= ta // 2 < limit
    R = np.zeros_like(passm)
    R[passm] = reached[rid[passm]]
    return R | seed, rounds


# ----------------------------------------------------------------------------------------------------------------------
# the region stages on top of it (structure only; the CPU test compares them with scipy)
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class RegionModel:
    """fill / component test of one mask as the kernel structures them.  ``wrong``: None or one of the deliberate faults
    'chunk' (no link across region word 64 / 128), 'bands', 'diag', 'seed' (right-border seed from W & 31), 'margin' (e - 1);
    ``limit``: None (run to the end), 'legacy' or 'proven'.  ``nw``: override the variant's wave count."""
    wrong: Optional[str] = None
    limit: Optional[str] = None
    nw: Optional[int] = None

    def _setup(self, mask: np.ndarray, box: Box, e: int):
        H, W = mask.shape
        if self.wrong == "margin":
            e -= 1
        ry0, wx0, rh, rw = region_of(box, e, H, W)
        xs0, xs1 = wx0 * 32, min((wx0 + rw) * 32, W)
        A = np.zeros((rh, 32 * rw), dtype=bool)
        A[:, :xs1 - xs0] = mask[ry0:ry0 + rh, xs0:xs1]
        nw = self.nw or waves(rh * rw)
        lim = {None: None, "legacy": legacy_max_rounds(rh, rw), "proven": proven_max_rounds(rh, rw)}[self.limit]
        kw = dict(rpb=-(-rh // nw), limit=lim, band_links=self.wrong != "bands", diag_across_words=self.wrong != "diag",
                  split_cols=[k * 32 for k in (64, 128, 192) if k < rw] if self.wrong == "chunk" else ())
        return (ry0, xs0, xs1, rh, rw, wx0), A, kw

    def _outside(self, A: np.ndarray, geo, box: Box, H: int, W: int, kw) -> Tuple[np.ndarray, int]:
        ry0, xs0, _, rh, rw, wx0 = geo
        cy0, cx0, cy1, cx1 = box
        ys = ry0 + np.arange(rh)[:, None]
        xs = xs0 + np.arange(32 * rw)[None, :]
        wpr = (W + 31) >> 5
        first_right = (wpr - 1) * 32 + ((W & 31) if self.wrong == "seed" else ((W - 1) & 31))    # pixel W - 1 and the padding bits
        seed = (ys < cy0) | (ys > cy1) | (ys == 0) | (ys == H - 1) | (xs < cx0) | (xs > cx1) | (xs == 0) | (xs >= first_right)
        return lockstep_flood(~A, ~A & seed, eight=False, **kw)

    def fill(self, mask: np.ndarray, box: Box, e: int = 1) -> Tuple[np.ndarray, int]:
        """(the mask after `fill`, rounds of the background flood)."""
        H, W = mask.shape
        if box == EMPTY:
            return mask.copy(), 0
        geo, A, kw = self._setup(mask, box, e)
        B, rounds = self._outside(A, geo, box, H, W, kw)
        ry0, xs0, xs1, rh, _, _ = geo
        out = mask.copy()
        out[ry0:ry0 + rh, xs0:xs1] = ~B[:, :xs1 - xs0]
        return out, rounds

    def multi(self, mask: np.ndarray, box: Box, e: int = 1) -> Tuple[bool, str, int]:
        """(more than one component, 'euler' | 'flood', rounds of the longest flood)."""
        H, W = mask.shape
        if box == EMPTY:
            return False, "empty", 0
        geo, A, kw = self._setup(mask, box, e)
        B, rounds = self._outside(A, geo, box, H, W, kw)
        if not (~(A | B)).any():
            p = np.pad(A, 1)
            a, b, c, d = p[:-1, :-1], p[:-1, 1:], p[1:, :-1], p[1:, 1:]
            s = a.astype(int) + b + c + d
            e4 = int((s == 1).sum()) - int((s == 3).sum()) - 2 * int(((a & d & ~b & ~c) | (b & c & ~a & ~d)).sum())
            return e4 > 4, "euler", rounds
        if not A.any():
            return False, "flood", rounds
        first = np.zeros_like(A)
        first.ravel()[int(np.flatnonzero(A.ravel())[0])] = True
        R, r8 = lockstep_flood(A, first, eight=True, **kw)
        return bool((R != A).any()), "flood", max(rounds, r8)
