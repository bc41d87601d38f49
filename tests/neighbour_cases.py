"""Hand-made scenes for the neighbour statistics (``demia_mask_neighbours``): dense masks ``[M, H, W]`` on frames whose width is
no multiple of 32, with masks that cross word boundaries, plus the group labels and the radius each scene is asked with, and --
where a value can be written down by hand -- the known answers (``known``: {(a, b): d2} and {a: nearest index}).

The two limits of ``csrc/neighbours.hip`` are restated here (``LDS_POINTS``, ``CAND_LIST``); ``test_cpu_neighbours.py`` parses
them out of the source, so a changed limit cannot leave ``combs`` and ``many_small`` below it silently.
"""
import re
from dataclasses import dataclass, field
from pathlib import Path
from typing import Dict, Optional, Tuple

import numpy as np

SOURCE = Path(__file__).resolve().parents[1] / "deepemia_amd" / "csrc" / "neighbours.hip"
LDS_POINTS = 8192        # border points of mask a staged in LDS; the rest is read from global memory
CAND_LIST = 256          # candidates kept in a per-block list; more than that are scanned again every step


def parse_limits() -> Tuple[int, int]:
    text = SOURCE.read_text()
    return tuple(int(re.search(rf"constexpr\s+int\s+{name}\s*=\s*(\d+)\s*;", text).group(1)) for name in ("NB_LDS_POINTS", "NB_CAND_LIST"))


@dataclass
class Scene:
    name: str
    masks: np.ndarray                        # [M, H, W] bool
    group: Optional[np.ndarray] = None       # [M] int32
    r2: int = -1
    known_d2: Dict[Tuple[int, int], int] = field(default_factory=dict)
    known_nearest: Dict[int, int] = field(default_factory=dict)      # a -> idx_any
    known_group_nearest: Dict[int, int] = field(default_factory=dict)

    @property
    def hw(self):
        return tuple(self.masks.shape[1:])


def _frame(M, H, W):
    return np.zeros((M, H, W), dtype=bool)


def _disc(H, W, cy, cx, r):
    y, x = np.mgrid[:H, :W]
    return (y - cy) ** 2 + (x - cx) ** 2 <= r * r


def adjacency():
    m = _frame(4, 40, 70)
    m[0, 10, 31] = True          # diagonal across the word boundary 31 | 32
    m[1, 11, 32] = True
    m[2, 20, 63] = True          # 4-adjacent across 63 | 64
    m[3, 20, 64] = True
    return Scene("adjacency", m, known_d2={(0, 1): 2, (1, 0): 2, (2, 3): 1, (3, 2): 1, (0, 2): 10 * 10 + 32 * 32},
                 known_nearest={0: 1, 1: 0, 2: 3, 3: 2})


def overlap_contained():
    m = _frame(4, 40, 70)
    m[0, 5:20, 10:45] = True
    m[1, 15:30, 40:69] = True    # partial overlap with 0
    m[2, 8:12, 30:36] = True     # contained in 0
    m[3, 35:38, 2:6] = True      # apart
    return Scene("overlap_contained", m, known_d2={(0, 1): 0, (0, 2): 0, (2, 0): 0, (1, 2): 4 * 4 + 5 * 5, (3, 0): 16 * 16 + 5 * 5},
                 known_nearest={0: 1, 2: 0, 3: 0})


def disc_in_hole():
    H, W = 70, 100
    m = _frame(3, H, W)
    m[0] = _disc(H, W, 35, 50, 30) & ~_disc(H, W, 35, 50, 20)     # a ring: its box contains mask 1, its pixels do not
    m[1] = _disc(H, W, 35, 50, 6)
    m[2, 0:3, 97:100] = True
    return Scene("disc_in_hole", m, known_d2={}, known_nearest={1: 0})


def tie_lower_index_wins():
    m = _frame(6, 70, 100)
    m[0, 66:69, 2:5] = True      # fillers, far from everything that matters
    m[1, 30, 50] = True          # a
    m[2, 30, 40] = True          # d2 = 100, box gap 100
    m[3, 2:4, 90:99] = True
    m[4, 60:64, 88:99] = True
    m[5, 24, 42] = True          # d2 = 36 + 64 = 100 as well, but the box reaches (10, 49): gap 36 + 1 -- visited FIRST, index higher
    m[5, 10, 49] = True
    return Scene("tie_lower_index_wins", m, known_d2={(1, 2): 100, (1, 5): 100}, known_nearest={1: 2})


def tie_symmetric():
    m = _frame(3, 40, 70)
    m[0, 18:22, 10:14] = True
    m[1, 18:22, 33:37] = True    # 20 columns from both
    m[2, 18:22, 56:60] = True
    return Scene("tie_symmetric", m, known_d2={(1, 0): 400, (1, 2): 400}, known_nearest={1: 0, 0: 1, 2: 1})


def edges_corners():
    H, W = 40, 70
    m = _frame(7, H, W)
    m[0, 0:3, 0:3] = True
    m[1, 0:2, W - 2:W] = True                # the last word holds 6 columns
    m[2, H - 3:H, 0:2] = True
    m[3, H - 1, W - 1] = True
    m[4, 0, 20:50] = True                    # along the top edge, across a word boundary
    m[5, 10:30, W - 1] = True                # along the right edge
    m[6, 15:25, 0] = True
    return Scene("edges_corners", m, known_d2={(0, 4): 18 * 18, (1, 5): 9 * 9, (3, 5): 10 * 10, (0, 1): 66 * 66})


def empty_among():
    m = _frame(5, 40, 70)
    m[0, 5:9, 5:9] = True
    m[2, 5:9, 12:20] = True      # 1 and 3 stay empty
    m[4, 30:33, 40:66] = True
    return Scene("empty_among", m, group=np.array([0, 0, 1, 1, 0], dtype=np.int32), r2=9, known_d2={(0, 2): 16},
                 known_nearest={0: 2, 2: 0}, known_group_nearest={0: 4, 2: -1})


def single():
    m = _frame(1, 40, 70)
    m[0, 10:20, 20:50] = True
    return Scene("single", m, r2=100, known_nearest={0: -1})


def groups_differ():
    m = _frame(5, 70, 100)
    m[0, 30:40, 30:40] = True
    m[1, 30:40, 43:50] = True    # nearest of 0, other group
    m[2, 30:40, 5:15] = True     # nearest of 0 in its own group
    m[3, 60:65, 60:95] = True
    m[4, 2:6, 60:95] = True
    return Scene("groups_differ", m, group=np.array([7, 3, 7, 3, 7], dtype=np.int32), r2=16, known_d2={(0, 1): 16, (0, 2): 256},
                 known_nearest={0: 1}, known_group_nearest={0: 2, 1: 3})


def interlocking_ls():
    """Two L shapes whose boxes overlap almost entirely while their pixels stay far apart, and a small mask whose box is further
    from mask 0 than the other L's (gap 0) but whose pixels are nearer: the pruning trap."""
    H, W = 70, 100
    m = _frame(3, H, W)
    m[0, 5:60, 5:8] = True       # | and _ of the first L
    m[0, 57:60, 5:90] = True
    m[1, 8:11, 20:95] = True     # the second, turned round
    m[1, 8:45, 92:95] = True
    m[2, 30:33, 20:23] = True
    return Scene("interlocking_ls", m, r2=144, known_d2={(0, 1): 13 * 13, (0, 2): 13 * 13, (2, 1): 20 * 20}, known_nearest={0: 1, 2: 0})


def gap_not_nearest():
    """The smallest box gap is not the nearest mask: a diagonal line whose box all but touches mask 0, with its pixels far away."""
    H, W = 70, 100
    m = _frame(3, H, W)
    m[0, 40:50, 10:20] = True
    for k in range(30):          # from (8, 22) to (37, 51), away from mask 0: box rows 8 .. 37, columns 22 .. 51, gap to mask 0 = 9 + 9
        m[1, 8 + k, 22 + k] = True
    m[2, 40:50, 26:30] = True    # box gap 49, and that is its distance
    return Scene("gap_not_nearest", m, known_d2={(0, 2): 49}, known_nearest={0: 2})


def radius_on(r2=13 * 13):
    m = _frame(3, 40, 70)
    m[0, 5:10, 5:10] = True
    m[1, 14:20, 21:30] = True    # dy 5, dx 12: d2 = 169
    m[2, 30:35, 60:68] = True
    return Scene(f"radius_{r2}", m, r2=r2, known_d2={(0, 1): 169})


def long_row():
    m = _frame(2, 1, 47000)
    m[0, 0, 0] = True
    m[1, 0, 46999] = True
    return Scene("long_row", m, r2=46999 * 46999, known_d2={(0, 1): 46999 * 46999}, known_nearest={0: 1, 1: 0})


N_SMALL = 600


def many_small(r2=50, name="many_small"):
    """600 masks of 1 to 4 pixels on 128 x 160: the first scan of every block meets more candidates than the list holds."""
    rng = np.random.default_rng(20260)
    H, W = 128, 160
    m = _frame(N_SMALL, H, W)
    for k in range(N_SMALL):
        y, x = int(rng.integers(0, H - 1)), int(rng.integers(0, W - 1))
        cells = [(0, 0), (0, 1), (1, 0), (1, 1)]
        for j in rng.permutation(4)[: int(rng.integers(1, 5))]:
            m[k, y + cells[j][0], x + cells[j][1]] = True
    return Scene(name, m, group=rng.integers(0, 3, N_SMALL).astype(np.int32), r2=r2)


def combs():
    """A one-pixel comb over 260 x 260 (every pixel a border pixel, four times the LDS staging limit) with two notches cut out, and a
    small second comb and a dot inside the notches: one near the comb's first rows, one far down its point list."""
    H = W = 260
    m = _frame(3, H, W)
    m[0, :, 0:W:2] = True
    m[0, 100:141, 100:161] = False
    m[0, 8:31, 190:231] = False
    m[1, 110:131, 112:150:3] = True          # the second comb: teeth three apart
    m[2, 19, 209] = True
    return Scene("combs", m, r2=100, known_d2={(2, 0): 12 * 12 + 1, (1, 0): 11 * 11})


def all_scenes():
    return [adjacency(), overlap_contained(), disc_in_hole(), tie_lower_index_wins(), tie_symmetric(), edges_corners(), empty_among(),
            single(), groups_differ(), interlocking_ls(), gap_not_nearest(), radius_on(169), radius_on(168), long_row(), many_small(),
            many_small(128 * 128 + 160 * 160, "many_small_all_within"), combs()]


def by_name():
    return {s.name: s for s in all_scenes()}


RANDOM_SEEDS = list(range(64))


def random_scene(seed: int, H: int = 96, W: int = 130) -> Scene:
    """2 to 40 blobs (discs, boxes, thin lines; they may overlap or contain one another), random groups, a radius from a few."""
    rng = np.random.default_rng(1000 + seed)
    M = int(rng.integers(2, 41))
    m = _frame(M, H, W)
    for k in range(M):
        kind = int(rng.integers(0, 4))
        cy, cx = int(rng.integers(0, H)), int(rng.integers(0, W))
        if kind == 0:
            m[k] = _disc(H, W, cy, cx, int(rng.integers(0, 9)))
        elif kind == 1:
            m[k, cy:cy + int(rng.integers(1, 12)), cx:cx + int(rng.integers(1, 40))] = True
        elif kind == 2:
            m[k] = _disc(H, W, cy, cx, int(rng.integers(6, 14))) & ~_disc(H, W, cy, cx, int(rng.integers(2, 6)))
        else:
            n = int(rng.integers(1, 30))
            dy, dx = int(rng.integers(-1, 2)), int(rng.integers(-1, 2))
            for t in range(n):
                y, x = cy + t * dy, cx + t * dx
                if 0 <= y < H and 0 <= x < W:
                    m[k, y, x] = True
    if seed % 7 == 3:
        m[int(rng.integers(0, M))] = False                       # an empty mask among them
    r2 = [-1, 0, 2, 30, 400, 5000][int(rng.integers(0, 6))]
    return Scene(f"random_{seed}", m, group=rng.integers(0, 3, M).astype(np.int32), r2=r2)
