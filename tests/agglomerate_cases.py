"""Hand-made scenes for the agglomerate statistics (``demia_mask_agglomerates``): small dense masks ``[M, H, W]`` with the group
labels, the link threshold ``l2`` and, where one matters, the ``label_lds_cap`` each is asked with, plus -- where it can be
written down by hand -- the partition (``known_parts``: the components as sets of indices).

The limits of ``csrc/agglomerates.hip`` are restated here; ``test_cpu_agglomerates.py`` parses
them out of the sources, so a changed limit cannot leave ``long_border`` below it silently.
"""
import re
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Set

import numpy as np

import neighbour_cases as NC

CSRC = Path(__file__).resolve().parents[1] / "deepemia_amd" / "csrc"
LDS_POINTS = 8192        # border points of mask a staged in LDS by the link kernel; the rest is read from global memory
NEAR = 256               # points of a near b's box kept in LDS; a pair with more runs over all of a's points
OWN_LIST = 64            # linked lower masks the own kernel lists in LDS; a mask with more scans its row for every word
LABEL_LDS = 8192         # labels the component kernel holds in LDS by default
MAX_M = 32768
MAX_HW = 32767


def parse_limits() -> dict:
    agg = (CSRC / "agglomerates.hip").read_text()

    def num(text, name, kind):
        return int(re.search(rf"constexpr\s+{kind}\s+{name}\s*=\s*(\d+)\s*;", text).group(1))
    return {"LDS_POINTS": num(agg, "AG_LDS_POINTS", "int"), "NEAR": num(agg, "AG_NEAR", "int"), "OWN_LIST": num(agg, "AG_OWN_LIST", "int"), "LABEL_LDS": num(agg, "AG_LABEL_LDS", "int"),
            "MAX_M": num(agg, "AG_MAX_M", "long"), "MAX_HW": num(agg, "AG_MAX_HW", "int")}


@dataclass
class Scene:
    name: str
    masks: np.ndarray                        # [M, H, W] bool
    group: Optional[np.ndarray] = None       # [M] int32
    l2: int = 2
    cap: int = 0                             # label_lds_cap
    known_parts: Optional[List[Set[int]]] = None


def _frame(M, H, W):
    return np.zeros((M, H, W), dtype=bool)


def pairs(l2):
    """Four pairs of 3 x 3 squares at d2 = 1, 2, 4 and 5, far from each other: which of them link depends on l2."""
    m = _frame(8, 60, 70)
    m[0, 2:5, 2:5] = True
    m[1, 2:5, 5:8] = True            # d2 = 1
    m[2, 2:5, 30:33] = True
    m[3, 5:8, 33:36] = True          # d2 = 2
    m[4, 30:33, 2:5] = True
    m[5, 30:33, 6:9] = True          # d2 = 4
    m[6, 30:33, 40:43] = True
    m[7, 33:36, 44:47] = True        # dx = 2, dy = 1: d2 = 5
    parts = [{0, 1}, {2, 3}] + ([{4, 5}] if l2 >= 4 else [{4}, {5}]) + ([{6, 7}] if l2 >= 5 else [{6}, {7}])
    return Scene(f"pairs_l2_{l2}", m, l2=l2, known_parts=parts)


def word_boundary():
    m = _frame(4, 40, 70)
    m[0, 10:13, 28:32] = True        # ends in column 31
    m[1, 10:13, 32:36] = True        # starts in column 32: 4-adjacent across 31 | 32
    m[2, 25, 31] = True
    m[3, 26, 32] = True              # diagonal across 31 | 32
    return Scene("word_boundary", m, known_parts=[{0, 1}, {2, 3}])


def last_column():
    m = _frame(3, 30, 70)            # 70 % 32 = 6
    m[0, 5:9, 66:70] = True          # in the last column
    m[1, 9:12, 62:66] = True         # diagonal to 0
    m[2, 20:24, 69] = True           # the last column alone
    return Scene("last_column", m, known_parts=[{0, 1}, {2}])


def corners_edges():
    H, W = 40, 70
    m = _frame(8, H, W)
    m[0, 0:2, 0:2] = True
    m[1, 0:2, W - 2:W] = True
    m[2, H - 2:H, 0:2] = True
    m[3, H - 2:H, W - 2:W] = True
    m[4, 0, 2:W - 2] = True          # the top edge between the corners: touches 0 and 1
    m[5, 2:H - 2, 0] = True          # the left edge: touches 0 and 2
    m[6, H - 1, 3:W - 3] = True      # the bottom edge, one pixel short of the corners
    m[7, 3:H - 3, W - 1] = True      # the right edge, likewise
    return Scene("corners_edges", m, known_parts=[{0, 1, 2, 4, 5}, {3}, {6}, {7}])


def overlaps():
    m = _frame(6, 60, 100)
    m[0, 5:20, 5:40] = True
    m[1, 10:25, 30:60] = True        # two overlapping
    m[2, 35:50, 10:50] = True
    m[3, 40:55, 30:70] = True
    m[4, 30:45, 40:60] = True        # three mutually overlapping: (40 .. 44, 40 .. 49) is shared by all
    m[5, 2:4, 90:95] = True
    return Scene("overlaps", m, known_parts=[{0, 1}, {2, 3, 4}, {5}])


def contained():
    m = _frame(3, 40, 70)
    m[0, 5:30, 10:60] = True
    m[1, 10:15, 28:36] = True        # inside 0, across the word boundary
    m[2, 35:38, 2:6] = True
    return Scene("contained", m, known_parts=[{0, 1}, {2}])


def disc_in_hole():
    H, W = 70, 100
    m = _frame(3, H, W)
    m[0] = NC._disc(H, W, 35, 50, 30) & ~NC._disc(H, W, 35, 50, 20)      # a ring: its box contains mask 1, its pixels do not
    m[1] = NC._disc(H, W, 35, 50, 6)
    m[2, 0:3, 97:100] = True
    return Scene("disc_in_hole", m, l2=5, known_parts=[{0}, {1}, {2}])


def empty_among():
    m = _frame(5, 40, 70)
    m[1, 5:9, 5:9] = True
    m[3, 9:12, 9:12] = True          # diagonal to 1
    m[4, 30:33, 60:64] = True
    return Scene("empty_among", m, known_parts=[{1, 3}, {4}])


def all_empty():
    return Scene("all_empty", _frame(4, 40, 70), known_parts=[])


def row_word_edges(M):
    """M single masks on a grid, far apart, except that 31 | 32 and 63 | 64 (where they exist) touch: the edges of the row words."""
    m = _frame(M, 96, 130)
    for k in range(M):
        y, x = 2 + 8 * (k // 13), 2 + 10 * (k % 13)
        m[k, y:y + 3, x:x + 3] = True
    parts = [{k} for k in range(M)]
    for a, b in ((31, 32), (63, 64)):
        if b < M:
            m[b] = False
            y, x = np.nonzero(m[a])
            m[b, y.max() + 1:y.max() + 3, x.max() + 1:x.max() + 3] = True        # diagonal to a
            parts = [p for p in parts if not (p & {a, b})] + [{a, b}]
    return Scene(f"row_word_edges_{M}", m, known_parts=parts)


def _serpentine(n, run):
    """Grid cells (row, col) of a path of n cells: runs of `run` cells on the even grid rows, joined at alternate ends by one cell on
    the odd row between them, so consecutive cells are 4-adjacent and runs two rows apart do not meet."""
    cells, r, c, step = [], 0, 0, 1
    while len(cells) < n:
        for _ in range(run):
            cells.append((r, c))
            c += step
        c -= step
        cells.append((r + 1, c))
        r += 2
        step = -step
    return cells[:n]


def _chain(m, first, cells, x0, order):
    for i, (r, c) in enumerate(cells):
        m[first + order[i], 2 * r:2 * r + 2, x0 + 2 * c:x0 + 2 * c + 2] = True


def chain(cap=0):
    """150 2 x 2 squares, each touching the next, indices by a fixed permutation: one component that label propagation crosses
    only in many rounds.  cap = 64 takes the labels out of LDS."""
    n = 150
    m = _frame(n, 30, 70)
    _chain(m, 0, _serpentine(n, 24), 1, np.random.default_rng(150).permutation(n))
    return Scene(f"chain_cap_{cap}", m, cap=cap, known_parts=[set(range(n))])


def two_chains(l2):
    """Two chains of 60 with one empty column between their nearest squares (d2 = 4)."""
    n = 60
    m = _frame(2 * n, 30, 100)
    order = np.random.default_rng(60).permutation(n)
    _chain(m, 0, _serpentine(n, 14), 0, order)                 # columns 0 .. 27
    _chain(m, n, _serpentine(n, 14), 29, order[::-1])          # columns 29 ..
    parts = [set(range(2 * n))] if l2 >= 4 else [set(range(n)), set(range(n, 2 * n))]
    return Scene(f"two_chains_l2_{l2}", m, l2=l2, known_parts=parts)


def long_border():
    """A comb of one-pixel teeth -- every pixel a border pixel, more of them than the LDS staging holds -- with a square touching its
    far corner, one touching its first tooth and one a pixel too far away."""
    H, W = 96, 200
    m = _frame(4, H, W)
    m[0, 0, 0:190] = True
    m[0, 1:90, 0:190:2] = True       # 95 teeth of 89 pixels + the spine: 8645 border points
    m[1, 90:93, 189:192] = True      # diagonal to the last tooth's end (89, 188)
    m[2, 90:92, 0:2] = True          # under the first tooth
    m[3, 91:94, 100:103] = True      # (91, 100) below the tooth end (89, 100): d2 = 4
    assert int(m[0].sum()) > LDS_POINTS
    return Scene("long_border", m, known_parts=[{0, 1, 2}, {3}])


def interleaved(l2):
    """Two combs with interleaved teeth, one empty column between a tooth and the next of the other comb (d2 = 4) and nothing
    closer: every point of one is near the other's box -- more than the near list holds -- and at l2 = 2 no pair ends the search."""
    H, W = 40, 70
    m = _frame(2, H, W)
    m[0, 0, 0:66] = True
    m[0, 1:H - 3, 0:66:4] = True     # teeth at 0, 4, ..., 64 down to row H - 4
    m[1, H - 1, 2:68] = True
    m[1, 3:H - 1, 2:68:4] = True     # teeth at 2, 6, ..., 66 up to row 3: three rows from the other spine
    assert int(m[0].sum()) > 2 * NEAR and int(m[1].sum()) > 2 * NEAR
    return Scene(f"interleaved_l2_{l2}", m, l2=l2, known_parts=[{0, 1}] if l2 >= 4 else [{0}, {1}])


def many_lower():
    """70 small squares, half inside and half across the edge of one large rectangle of a HIGHER index: more linked lower masks
    than the own kernel lists."""
    n = 70
    m = _frame(n + 2, 40, 130)
    for k in range(n):
        y, x = (4, 12, 20, 28, 33)[k // 14], 6 + 8 * (k % 14)
        m[k, y:y + 3, x:x + 3] = True
    m[n, 6:35, 4:120] = True         # rows 6 .. 34: the squares at y = 4 and y = 33 stick out
    m[n + 1, 0:2, 126:130] = True
    assert n > OWN_LIST
    return Scene("many_lower", m, known_parts=[set(range(n + 1)), {n + 1}])


def classes(same):
    """Two classes interleaved along a row, each touching the next, and two overlapping masks of different classes: `any` joins
    what `same_class` splits; the shared pixels are then counted in both components."""
    m = _frame(8, 40, 100)
    for k in range(6):
        m[k, 5:9, 4 * k:4 * k + 4] = True
    m[6, 20:30, 10:40] = True
    m[7, 25:35, 30:60] = True        # overlaps 6, the other class
    group = np.array([0, 1, 0, 1, 0, 1, 0, 1], dtype=np.int32)
    parts = [{k} for k in range(8)] if same else [set(range(6)), {6, 7}]
    return Scene("classes_same" if same else "classes_any", m, group=group if same else None, known_parts=parts)


def all_scenes():
    return [pairs(2), pairs(4), pairs(5), word_boundary(), last_column(), corners_edges(), overlaps(), contained(), disc_in_hole(),
            empty_among(), all_empty(), row_word_edges(1), row_word_edges(33), row_word_edges(65), chain(0), chain(64), two_chains(2),
            two_chains(4), long_border(), interleaved(2), interleaved(4), many_lower(), classes(False), classes(True)]


def by_name():
    return {s.name: s for s in all_scenes()}


RANDOM_SEEDS = list(range(64))


def random_scene(seed: int) -> Scene:
    """The neighbour tests' random scene (M <= 40, discs, bars, rings, strokes, sometimes an empty mask) with a link threshold
    and, two times out of three, its groups."""
    s = NC.random_scene(seed)
    return Scene(f"random_{seed}", s.masks, group=None if seed % 3 == 0 else s.group, l2=[2, 2, 4, 5, 9, 30][seed % 6])
