"""Scenes for the error-map kernel (``csrc/errormap.hip``): the smallest frames at which it can still go wrong -- two whole tiles
and a partial one each way, for the tile the source states -- with masks on every seam and edge the kernel has, every interaction
between states the definitions name, lines wider than the masks, more masks on one tile than a ballot round takes, and empty sets.
Dense boolean masks; the tests pack them.  ``scenes()`` is deterministic; ``random_scene(seed)`` draws one more."""
import re
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np

SOURCE = Path(__file__).resolve().parents[1] / "deepemia_amd" / "csrc" / "errormap.hip"
OTHER_PALETTE = np.array([[10, 200, 30], [250, 3, 77], [1, 2, 3], [90, 91, 92], [255, 0, 128], [17, 170, 240], [64, 0, 0], [200, 100, 50]],
                         dtype=np.uint8)


def parse_tile() -> Tuple[int, int, int]:
    """(rows, word columns, masks per ballot round) of a tile, as the source states them."""
    text = SOURCE.read_text()

    def num(name):
        return int(re.search(rf"constexpr\s+int\s+{name}\s*=\s*(\d+)\s*;", text).group(1))
    threads = int(re.search(r"constexpr\s+int\s+THREADS\s*=\s*(\d+)", (SOURCE.parent / "wordregion.h").read_text()).group(1))
    return num("EM_ROWS"), num("EM_WORDS"), threads


@dataclass
class Scene:
    name: str
    det: np.ndarray              # [D, H, W] bool
    d_state: np.ndarray          # [D] int32
    gt: np.ndarray               # [G, H, W] bool
    g_state: np.ndarray          # [G] int32
    image: np.ndarray            # [H, W, C] uint8, C in {1, 3}
    alpha: int
    line: int
    palette: Optional[np.ndarray] = None

    @property
    def hw(self) -> Tuple[int, int]:
        return tuple(int(v) for v in self.image.shape[:2])


def frame_sizes() -> List[Tuple[int, int]]:
    """(H, W): two whole tiles and a partial one each way; widths with W % 32 in {0, 6, 31}."""
    rows, words, _ = parse_tile()
    tile_w = 32 * words
    return [(2 * rows + 11, 2 * tile_w + 32), (2 * rows + 5, 2 * tile_w + 6), (2 * rows + 1, 2 * tile_w + 31)]


def _rect(hw, y0, x0, y1, x1):
    m = np.zeros(hw, dtype=bool)
    m[max(y0, 0):y1 + 1, max(x0, 0):x1 + 1] = True
    return m


def _disc(hw, cy, cx, r):
    yy, xx = np.mgrid[:hw[0], :hw[1]]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def _image(seed, hw, C):
    return np.random.RandomState(seed).randint(0, 256, (hw[0], hw[1], C)).astype(np.uint8)


def _stack(masks, hw):
    return np.stack(masks).astype(bool) if masks else np.zeros((0,) + tuple(hw), dtype=bool)


def _scene(name, hw, dets, gts, C, alpha, line, palette=None, seed=0):
    return Scene(name, _stack([m for m, _ in dets], hw), np.asarray([s for _, s in dets], dtype=np.int32),
                 _stack([m for m, _ in gts], hw), np.asarray([s for _, s in gts], dtype=np.int32), _image(seed, hw, C), alpha, line, palette)


def _seams(hw):
    """Masks across the tile seams in both directions and across a word seam, on all four frame edges and in column W - 1, a single
    pixel, a full-frame mask, an empty mask among the others, and a state-0 mask over others."""
    rows, words, _ = parse_tile()
    H, W = hw
    tw = 32 * words
    dets = [(_rect(hw, rows - 6, tw - 9, rows + 7, tw + 12), 1),            # over the crossing of two tile seams
            (_rect(hw, 5, 27, 20, 36), 2),                                  # over the word seam x = 31 | 32
            (_rect(hw, 0, 40, 9, 60), 1),                                   # top edge
            (_rect(hw, H - 7, 300, H - 1, 330), 2),                         # bottom edge
            (_rect(hw, 30, 0, 45, 8), 1),                                   # left edge, over a tile seam in y
            (_rect(hw, 12, W - 10, 50, W - 1), 2),                          # right edge: column W - 1
            (_rect(hw, 22, 100, 22, 100), 2),                               # a single pixel
            (np.zeros(hw, dtype=bool), 1),                                  # empty: its box is -1
            (_rect(hw, 0, 0, H - 1, W - 1), 0),                             # not drawn, over everything
            (_disc(hw, 2 * rows + 1, 2 * tw - 3, 14), 1)]                   # over the seams into the partial tiles
    gts = [(_rect(hw, rows - 4, tw - 14, rows + 9, tw + 8), 1),
           (_rect(hw, 3, 29, 18, 40), 1),
           (_rect(hw, 0, 44, 11, 58), 2),
           (_rect(hw, 0, 0, H - 1, W - 1), 1),                              # a full-frame annotation
           (np.zeros(hw, dtype=bool), 2),
           (_rect(hw, 10, W - 1, 40, W - 1), 2),                            # a bar in column W - 1
           (_disc(hw, 40, 200, 25), 0),                                     # skipped
           (_rect(hw, H - 3, W - 40, H - 1, W - 1), 3)]                     # a crowd region in the corner
    return dets, gts


def _interactions(hw):
    """Nested and overlapping detections of different states; a crowd region under a detection and beside an annotation."""
    dets = [(_disc(hw, 30, 60, 24), 1), (_disc(hw, 30, 60, 10), 2), (_disc(hw, 34, 90, 18), 2), (_disc(hw, 30, 60, 17), 1),
            (_rect(hw, 10, 300, 50, 360), 2),                               # over a crowd region: ignored
            (_rect(hw, 20, 420, 44, 470), 1)]
    gts = [(_disc(hw, 32, 64, 22), 1), (_disc(hw, 36, 100, 12), 2),
           (_rect(hw, 5, 290, 40, 340), 3),                                 # the crowd region under the detection
           (_rect(hw, 22, 425, 46, 468), 1), (_rect(hw, 18, 469, 50, 500), 3),        # a crowd region beside (and touching) an annotation
           (_rect(hw, 30, 330, 60, 350), 2)]                                # an annotation inside crowd and detection: agree wins
    return dets, gts


def _thin(hw, t):
    """Bars of every width from 1 to 2t + 2, upright and lying: up to 2t they are all outline, from 2t + 1 on they have an interior."""
    dets, gts = [], []
    for k, w in enumerate(range(1, 2 * t + 3)):
        dets.append((_rect(hw, 4, 10 + 24 * k, 40, 10 + 24 * k + w - 1), 1 + k % 2))
        gts.append((_rect(hw, 45 + 0 * k, 6 + 24 * k, 45 + w - 1, 6 + 24 * k + 17), 1 + k % 3))
    return dets, gts


def _crowded_tile(hw):
    """More masks on one tile than a ballot round takes: 300 detections and 280 annotations of 1 x 2 pixels, all in the second tile of
    the first tile row, one beside the other with overlaps; the states alternate."""
    rows, words, per_round = parse_tile()
    assert 300 > per_round
    x_first = 32 * words + 3
    dets, gts = [], []
    for k in range(300):
        y, x = 1 + (k % 15) * 2, x_first + (k // 15) * 3
        dets.append((_rect(hw, y, x, y, x + 1), 1 + k % 2))
    for k in range(280):
        y, x = 1 + (k % 14) * 2, x_first + 1 + (k // 14) * 3
        gts.append((_rect(hw, y, x, y + (k % 2), x + 1), 1 + k % 3))
    return dets, gts


def scenes() -> List[Scene]:
    sizes = frame_sizes()
    out = []
    # the seam scenes, one per width: every C, alpha, line and palette is met once at least
    for k, (hw, C, alpha, line, pal) in enumerate(zip(sizes, (3, 1, 3), (96, 256, 0), (1, 2, 3), (None, OTHER_PALETTE, None))):
        out.append(_scene(f"seams_w{hw[1]}", hw, *_seams(hw), C, alpha, line, pal, seed=10 + k))
    out.append(_scene("interactions", sizes[1], *_interactions(sizes[1]), 3, 96, 2, seed=20))
    out.append(_scene("interactions_gray_other_palette", sizes[2], *_interactions(sizes[2]), 1, 96, 4, OTHER_PALETTE, seed=21))
    for t in (1, 2, 3, 4):
        out.append(_scene(f"thin_t{t}", sizes[t % 3], *_thin(sizes[t % 3], t), 3 if t % 2 else 1, (96, 256)[t % 2], t, seed=30 + t))
    out.append(_scene("crowded_tile", sizes[2], *_crowded_tile(sizes[2]), 3, 96, 1, seed=40))
    dets, gts = _interactions(sizes[0])
    out.append(_scene("no_detections", sizes[0], [], gts, 3, 96, 1, seed=50))
    out.append(_scene("no_annotations", sizes[0], dets, [], 1, 96, 2, seed=51))
    out.append(_scene("no_masks", sizes[1], [], [], 3, 96, 1, seed=52))
    out.append(_scene("no_masks_gray", sizes[2], [], [], 1, 256, 4, seed=53))
    return out


def random_scene(seed: int) -> Scene:
    rng = np.random.RandomState(1000 + seed)
    hw = frame_sizes()[seed % 3]
    H, W = hw

    def masks(n, top):
        out = []
        for _ in range(n):
            kind = rng.randint(0, 4)
            cy, cx = rng.randint(-5, H + 5), rng.randint(-5, W + 5)
            if kind == 0:
                m = _disc(hw, cy, cx, rng.randint(1, 30))
            elif kind == 1:
                m = _rect(hw, cy, cx, cy + rng.randint(0, 40), cx + rng.randint(0, 90))
            elif kind == 2:
                m = _disc(hw, cy, cx, rng.randint(3, 25)) & (rng.rand(H, W) < .7)          # ragged: holes and specks
            else:
                m = _rect(hw, cy, cx, cy + rng.randint(0, 9), cx + rng.randint(0, 9))
            out.append((m, int(rng.randint(0, top + 1))))
        return out
    return _scene(f"random_{seed}", hw, masks(rng.randint(0, 14), 2), masks(rng.randint(0, 14), 3), int(rng.choice([1, 3])),
                  int(rng.choice([0, 96, 256, rng.randint(0, 257)])), int(rng.randint(1, 5)), OTHER_PALETTE if seed % 4 == 3 else None,
                  seed=2000 + seed)
