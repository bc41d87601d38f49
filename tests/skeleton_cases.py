"""The masks the skeleton-descriptor tests run on (``test_cpu_skeleton.py``, ``test_gpu_skeleton.py``): every mask of
``inscribed_cases.py`` -- they reach one pixel, the frame-filling region, the partial last word, a word boundary, the flood's
general loop beyond 64 words, the scratch path beyond the tracer's large LDS buffer, nested components and more contours than the
fetch slots -- and the shapes a skeleton is asked about: lines, bars, discs, rings, junctions, bands, with the known answers of the
definition."""
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

import inscribed_cases as IC


class Case(NamedTuple):
    name: str
    mask: np.ndarray                              # [H, W] bool
    contours: int                                 # external contours (components not nested in a hole); -1: not stated
    known: Optional[Tuple[Tuple[int, int, int, int, int], ...]] = None      # (n, n4, nd, ends, branches) per contour, raster order of the start


LARGE = IC.LARGE                                  # region beyond the tracer's large LDS buffer: the scratch path
WIDE = IC.WIDE                                    # more than 64 words wide: the flood's general loop


def _frame(h, w):
    return np.zeros((h, w), dtype=bool)


def disc18():
    yy, xx = np.mgrid[0:41, 0:41]
    return (yy - 20) ** 2 + (xx - 20) ** 2 <= 18 ** 2


def ring18():
    yy, xx = np.mgrid[0:41, 0:41]
    return disc18() & ~((yy - 20) ** 2 + (xx - 20) ** 2 <= 9 ** 2)


def plus41():
    m = _frame(41, 41)
    m[18:23, :] = True
    m[:, 18:23] = True
    return m


def ellipse_140x60():
    yy, xx = np.mgrid[0:125, 0:285]
    return ((xx - 142) / 140.0) ** 2 + ((yy - 62) / 60.0) ** 2 < 1.0


def _known() -> List[Case]:
    one = _frame(7, 9); one[4, 6] = True
    blk = _frame(8, 8); blk[3:5, 3:5] = True
    line = _frame(5, 13); line[2, 2:11] = True
    bar = _frame(6, 13); bar[2:4, 2:11] = True
    rect = _frame(11, 35); rect[2:9, 2:33] = True
    return [Case("k_one_pixel", one, 1, ((1, 0, 0, 0, 0),)),
            Case("k_block2x2", blk, 1, ((1, 0, 0, 0, 0),)),
            Case("k_line1x9", line, 1, ((9, 8, 0, 2, 0),)),
            Case("k_bar2x9", bar, 1, ((8, 7, 0, 2, 0),)),
            Case("k_rect7x31", rect, 1, ((25, 24, 0, 2, 0),)),
            Case("k_disc18", disc18(), 1, ((3, 2, 0, 2, 0),)),
            Case("k_ring18_9", ring18(), 1, ((74, 40, 34, 0, 0),)),
            Case("k_plus41", plus41(), 1, ((73, 72, 0, 4, 1),)),
            Case("k_ellipse140x60", ellipse_140x60(), 1, ((192, 191, 0, 2, 0),))]


KNOWN = tuple(c.name for c in _known())
ELLIPSE_PAIRS = 60                                # pairs of sub-iterations the ellipse takes, the last (empty) one included


def cases() -> List[Case]:
    out = [Case(c.name, c.mask, c.contours) for c in IC.cases()]
    out += _known()
    yy, xx = np.mgrid[0:70, 0:100]
    out.append(Case("band_diagonal", (np.abs((xx - 10) - (yy - 5) * 1.3) <= 6) & (yy >= 4) & (yy <= 65) & (xx >= 3) & (xx <= 96), 1))
    m = _frame(50, 80); m[5:10, 8:72] = True; m[10:45, 37:42] = True
    out.append(Case("junction_T", m, 1))
    m = _frame(70, 90)
    for k in range(30):                               # two 5-px arms running down to the centre, one stem below it
        m[5 + k:9 + k, 12 + k:17 + k] = True
        m[5 + k:9 + k, 72 - k:77 - k] = True
    m[34:65, 42:47] = True
    out.append(Case("junction_Y", m, 1))
    m = _frame(30, 70); m[4:26, 30:35] = True         # five pixels wide, two in word 0 and three in word 1
    out.append(Case("bar_cols_30_34", m, 1))
    m = _frame(30, 70); m[4:26, 31:33] = True         # two pixels wide, one on each side of the word boundary
    out.append(Case("bar_cols_31_32", m, 1))
    m = _frame(37, 67); m[16:21, :] = True; m[:, 29:35] = True; m[0, :] = True; m[-1, :] = True; m[:, 0] = True; m[:, -1] = True
    out.append(Case("frame_and_cross_touch_all_edges", m, 1))
    assert len({c.name for c in out}) == len(out)
    return out


def by_name() -> Dict[str, Case]:
    return {c.name: c for c in cases()}
