"""The masks the inscribed-descriptor tests run on (``test_cpu_inscribed.py``, ``test_gpu_inscribed.py``): small frames that reach
every path of ``mask_inscribed_kernel`` -- one pixel to a frame-filling region, the partial last word, a word boundary, the flood's
general loop beyond 64 words, the block-wide row buffer beyond 1024 region pixels, the scratch path beyond the tracer's large LDS
buffer, ties of the centre, nested components, more contours than the fetch slots."""
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from mask_region_cases import serpentine


class Case(NamedTuple):
    name: str
    mask: np.ndarray                              # [H, W] bool
    contours: int                                 # external contours (components not nested in a hole)
    known: Optional[Tuple[Tuple[int, int, int, int, int], ...]] = None      # (R2, cx, cy, N, SD2) per contour, in raster order of the start
    small: bool = False                           # small enough for the brute-force D2


def _frame(h, w):
    return np.zeros((h, w), dtype=bool)


def disc(h=61, w=61, cy=30, cx=30, r2=400):
    yy, xx = np.mgrid[0:h, 0:w]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r2


def ring():
    yy, xx = np.mgrid[0:61, 0:61]
    return disc() & ~((yy - 30) ** 2 + (xx - 30) ** 2 < 100)


def cleared_frame():
    m = np.ones((320, 1000), dtype=bool)
    m[100:110, 500:1000] = False
    return m


def six_components():
    """Six components of different shapes in one mask: more contours than the four fetch slots."""
    m = _frame(90, 150)
    m[3:20, 4:30] = True
    m[30:37, 5:60] = True
    m[50:85, 10:40] = True
    yy, xx = np.mgrid[0:90, 0:150]
    m |= (yy - 20) ** 2 + (xx - 80) ** 2 <= 15 ** 2
    m |= ((xx - 110) * 0.8 + (yy - 60) * 0.6) ** 2 / 30 ** 2 + (-(xx - 110) * 0.6 + (yy - 60) * 0.8) ** 2 / 9 ** 2 <= 1
    m[5, 140] = True
    return m


def noise_blob(fill, seed):
    return np.random.default_rng(seed).random((48, 48)) < fill


def _known():
    one = _frame(7, 9)
    one[4, 6] = True
    full = np.ones((5, 9), dtype=bool)
    rect = _frame(9, 13)
    rect[2:6, 2:11] = True
    return [Case("one_pixel", one, 1, ((1, 6, 4, 1, 1),), True),
            Case("rect5x9_fills_frame", full, 1, ((9, 2, 2, 45, 133),), True),
            Case("rect4x9", rect, 1, ((4, 3, 3, 36, 78),), True),
            Case("disc", disc(), 1, ((401, 30, 30, 1257, 87661),)),
            Case("ring", ring(), 1, ((29, 21, 18, 952, 9904),)),
            Case("cleared_320x1000", cleared_frame(), 1, ((25600, 159, 159, 315000, 1397852109),))]


KNOWN = tuple(c.name for c in _known())
LARGE = "cleared_320x1000"                        # region beyond the tracer's large LDS buffer: the scratch path
WIDE = "bar_24x2208"                              # more than 64 words wide: the flood's general loop, the block-wide row buffer


def cases() -> List[Case]:
    out = _known()
    m = _frame(9, 40); m[4, 3:37] = True
    out.append(Case("line_horizontal", m, 1, small=True))
    m = _frame(40, 9); m[3:37, 4] = True
    out.append(Case("line_vertical", m, 1, small=True))
    m = _frame(40, 40); m[np.arange(3, 37), np.arange(3, 37)] = True
    out.append(Case("line_diagonal", m, 1, small=True))
    m = _frame(8, 8); m[3:5, 3:5] = True
    out.append(Case("block2x2", m, 1, small=True))
    m = _frame(20, 30); m[4:15, 5:20] = True             # 11 x 15: one centre
    out.append(Case("rect_odd", m, 1, small=True))
    m = _frame(20, 30); m[4:16, 5:21] = True             # 12 x 16: a plateau of centres, the tie rule picks the raster-first
    out.append(Case("rect_even", m, 1, small=True))
    m = _frame(20, 30); m[4:14, 5:22] = True             # 10 x 17: a row pair of ties
    out.append(Case("rect_even_odd", m, 1, small=True))
    yy, xx = np.mgrid[0:120, 0:160]
    m = ((xx - 80) * 0.8 + (yy - 60) * 0.6) ** 2 / 60 ** 2 + (-(xx - 80) * 0.6 + (yy - 60) * 0.8) ** 2 / 25 ** 2 <= 1
    out.append(Case("ellipse_rotated", m, 1))
    m = _frame(70, 70); m[5:65, 5:65] = True; m[25:45, 25:45] = False; m[34:36, 45:65] = False
    out.append(Case("c_shape", m, 1))                    # a C with a 2-px slit: for the arms' ends the nearest background lies in the opening
    yy, xx = np.mgrid[0:80, 0:200]
    m = ((yy - 40) ** 2 + (xx - 40) ** 2 <= 30 ** 2) | ((yy - 40) ** 2 + (xx - 150) ** 2 <= 22 ** 2)
    m[37:44, 40:150] = True
    out.append(Case("dumbbell", m, 1))
    m = _frame(60, 100); m[5:40, 5:30] = True; m[20:28, 50:95] = True
    out.append(Case("two_components", m, 2))
    m = ring().copy(); m[27:34, 27:34] = True            # a component in the ring's hole: no row, foreground for D2
    out.append(Case("nested_in_ring", m, 1))
    out.append(Case("touches_all_edges", disc(41, 53, 20, 26, 30 ** 2), 1))
    m = _frame(30, 70); m[3:27, 50:70] = True            # W = 70: pixels in the last, partial word
    out.append(Case("partial_last_word", m, 1))
    m = _frame(20, 70); m[4:16, 30:35] = True            # columns 30..34: two words
    out.append(Case("word_boundary_30_34", m, 1, small=True))
    m = _frame(24, 2208); m[6:18, 40:2200] = True        # a bar 2160 px = 68 words wide
    out.append(Case(WIDE, m, 1))
    m = _frame(40, 120); m[3:33, 33:103] = serpentine(30, 70)
    out.append(Case("serpentine_30x70", m, 1))
    out.append(Case("noise_0.6", noise_blob(0.6, 11), -1, small=True))
    out.append(Case("noise_0.9", noise_blob(0.9, 12), -1, small=True))
    out.append(Case("six_components", six_components(), 6))
    assert len({c.name for c in out}) == len(out)
    return out


def by_name() -> Dict[str, Case]:
    return {c.name: c for c in cases()}
