"""The case tables of the tile-merge edge suite: tile placement (``demia_mask_place_tiles``, ``demia_crop_place_tiles``,
``cropset.rooms_of_placed_tiles``), score-ordered overlap removal (``demia_mask_overlap_prefix``) and per-column counts
(``demia_mask_column_counts``).  Importable without a GPU; every random draw comes from a seed derived from the case's name.
The references are ``merge_ref.py``; ``test_cpu_merge_ref.py`` checks the tables' own conditions (which sizes tell a wrong index
rule from the right one and where that shows, how often masks chain over one pixel, the size caps) and
``test_gpu_merge_edges.py`` runs the kernels on them.

Placement.  The kernels' index rule is cv2's INTER_NEAREST in float64, ``min(floor(t * (1 / (dst / src))), src - 1)``.  At an
exact 2x, at 1.5x and at most of the pipeline's own sizes it gives what ``t * src // dst``, ``t * (src / dst)`` and the float32
form of itself give; at the TELLTALE pairs below it differs from all three at one index or more, and a one-pixel checkerboard
makes every wrong source index flip a pixel.
"""
import functools
import zlib
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

import merge_ref as REF

MAX_FRAME = (200, 330)
MAX_T = 12


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


# ------------------------------------------------------------------------------------------------------------------
# placement
# ------------------------------------------------------------------------------------------------------------------
# (dst, src) at which the float64 rule differs from the integer rule, from the direct ratio AND from its float32 form
TELLTALE_UP = [(50, 44), (52, 40), (54, 42), (55, 45)]
TELLTALE_DOWN = [(40, 52), (40, 72), (40, 104), (40, 148)]
TELLTALE = TELLTALE_UP + TELLTALE_DOWN
SCALES = (0.5, 0.6, 0.7, 1.5, 2.0, 2.5)                 # inference.py: the multi-scale path's scales
MULTISCALE_FRAMES = ((100, 130), (90, 77))

KINDS = ("random", "checker", "ones", "empty", "corner_tl", "corner_tr", "corner_bl", "corner_br")


def source_mask(kind: str, sh: int, sw: int, rng) -> np.ndarray:
    m = np.zeros((sh, sw), dtype=bool)
    if kind == "random":
        m = rng.random((sh, sw)) < 0.5
    elif kind == "checker":
        m = ((np.arange(sh)[:, None] + np.arange(sw)[None, :]) & 1).astype(bool)
    elif kind == "ones":
        m[:] = True
    elif kind.startswith("corner_"):
        m[0 if kind[7] == "t" else sh - 1, 0 if kind[8] == "l" else sw - 1] = True
    else:
        assert kind == "empty", kind
    return m


@dataclass(frozen=True)
class PlaceCase:
    name: str
    src: Tuple[int, int]                    # (sh, sw) of the tile masks
    tile: Tuple[int, int]                   # (tile_h, tile_w) they are resized to
    frame: Tuple[int, int]                  # (H, W)
    offsets: Tuple[Tuple[int, int], ...]    # (xo, yo) per tile
    kinds: Tuple[str, ...]                  # mask generator per tile
    telltale: bool = False                  # both size pairs are TELLTALE pairs: every wrong rule must change a placed pixel

    @property
    def T(self) -> int:
        return len(self.offsets)

    @property
    def xo(self) -> List[int]:
        return [o[0] for o in self.offsets]

    @property
    def yo(self) -> List[int]:
        return [o[1] for o in self.offsets]

    def size_pairs(self):
        """(dst, src) per axis, y first."""
        return ((self.tile[0], self.src[0]), (self.tile[1], self.src[1]))


@functools.lru_cache(maxsize=None)
def _sources(name: str) -> np.ndarray:
    c = PLACE_BY_NAME[name]
    rng = _rng(name)
    out = np.zeros((c.T,) + c.src, dtype=bool)
    for t, k in enumerate(c.kinds):
        out[t] = source_mask(k, c.src[0], c.src[1], rng)
    out.setflags(write=False)
    return out


def sources(c: PlaceCase) -> np.ndarray:
    """bool [T, sh, sw], read-only."""
    return _sources(c.name)


def packed_sources(c: PlaceCase) -> np.ndarray:
    """uint32 [T, sh, ceil(sw / 32)] with the padding bits of every row's last word SET: the kernels clamp the source column
    to sw - 1, so these bits must never reach the frame."""
    return REF.pack(sources(c), c.src[1], pad_ones=True)


@functools.lru_cache(maxsize=None)
def _placed(name: str, rule: str) -> np.ndarray:
    c = PLACE_BY_NAME[name]
    fn = REF.nearest_rule if rule == "f64" else REF.WRONG_RULES[rule]
    H, W = c.frame
    out = np.zeros((c.T, H, W), dtype=bool)
    for t in range(c.T):
        out[t] = REF.place(sources(c)[t], c.tile[0], c.tile[1], c.offsets[t][0], c.offsets[t][1], H, W, rule=fn)
    out.setflags(write=False)
    return out


def placed(c: PlaceCase) -> np.ndarray:
    """The reference result bool [T, H, W], computed once per case and read-only."""
    return _placed(c.name, "f64")


def wrong_rule_pixels(c: PlaceCase) -> dict:
    """Per wrong rule: how many placed pixels of the case would differ if the kernel used it."""
    return {k: int((_placed(c.name, k) != placed(c)).sum()) for k in REF.WRONG_RULES}


def source_boxes(c: PlaceCase) -> np.ndarray:
    """Tight boxes int32 [T, 4] of the source masks (-1: empty)."""
    return np.array([REF.area_bbox(m)[1] for m in sources(c)], dtype=np.int32).reshape(c.T, 4)


def grow_boxes(boxes: np.ndarray, hw, by=(3, 33, 2, 40)) -> np.ndarray:
    """Boxes grown by (up, left, down, right) pixels and clipped to the frame ``hw``; -1 stays -1."""
    b = np.asarray(boxes, dtype=np.int64).reshape(-1, 4).copy()
    ok = b[:, 0] >= 0
    b[ok, 0] = np.maximum(b[ok, 0] - by[0], 0)
    b[ok, 1] = np.maximum(b[ok, 1] - by[1], 0)
    b[ok, 2] = np.minimum(b[ok, 2] + by[2], hw[0] - 1)
    b[ok, 3] = np.minimum(b[ok, 3] + by[3], hw[1] - 1)
    return b.astype(np.int32)


def _cycle(seq, n):
    return tuple(seq[i % len(seq)] for i in range(n))


def _resize_case(name, src, tile, frame, telltale=False) -> PlaceCase:
    """Eight tiles, one per mask kind, at offsets that are word-aligned and not, cut at the left and at the top, and that
    end exactly at the frame's last column and row; the first two (random, checkerboard) lie wholly inside the frame."""
    (th, tw), (H, W) = tile, frame
    assert H >= th and W >= tw
    dx, dy = W - tw, H - th
    offs = [(0, 0), (min(1, dx), 0), (min(31, dx), min(2, dy)), (min(32, dx), -3), (min(33, dx), min(5, dy)), (-5, min(1, dy)), (dx, dy),
            (dx + 9, 0)]
    return PlaceCase(name, src, tile, frame, tuple(offs), KINDS, telltale)


def _geometry(H, W, th, tw):
    """Two offset lists for a (th, tw) tile in an (H, W) frame: A inside and across the edges, B outside, cut and one pixel."""
    a = [(0, 0), (1, 2), (31, 3), (32, 0), (33, 5), (63, 1),
         (W - tw + 7, 4), (3, H - th + 9), (W - tw + 5, H - th + 6),             # across the right edge, the bottom edge, both
         (W - tw, 2), (2, H - th)]                                               # ending exactly at column W - 1 / row H - 1
    b = [(W, 0), (W + 40, 3), (0, H), (-tw, 0), (-tw - 5, 2), (0, -th),          # wholly outside
         (-7, -9), (-33, 0), (0, -1),                                            # the tile's first rows and columns cut
         (-tw + 1, 3),                                                           # only the tile's last column, at x = 0
         (W - 1, 0),                                                             # one tile column in the frame's last word
         (W - 1, H - 1)]                                                         # one pixel
    return a, b


def _place_cases() -> List[PlaceCase]:
    cases = [
        _resize_case("identity_64", (64, 64), (64, 64), (80, 130)),
        _resize_case("half_128_to_64", (128, 128), (64, 64), (70, 192)),
        _resize_case("undo_upscale_96_to_64", (96, 96), (64, 64), (64, 97)),
        _resize_case("undo_upscale_300_to_200", (300, 300), (200, 200), (200, 230)),
    ]
    # the multi-scale path: whole-frame resizes with src_w = int(w * s)
    for (h, w) in MULTISCALE_FRAMES:
        for s in SCALES:
            cases.append(PlaceCase(f"multiscale_{h}x{w}_s{s}", (int(h * s), int(w * s)), (h, w), (h, w), ((0, 0),) * len(KINDS), KINDS))
    # tell-tale pairs: the same pair on both axes, then mixed (enlarging on one axis, shrinking on the other: unequal ratios)
    for d, s in TELLTALE:
        cases.append(_resize_case(f"telltale_{s}_to_{d}", (s, s), (d, d), (d + 11, d + 45 if d != 50 else 96), telltale=True))
    for (dy, sy), (dx, sx) in (((50, 44), (40, 104)), ((40, 72), (55, 45)), ((54, 42), (52, 40)), ((40, 148), (40, 52))):
        cases.append(_resize_case(f"telltale_y{sy}_to_{dy}_x{sx}_to_{dx}", (sy, sx), (dy, dx), (dy + 3, dx + 37), telltale=True))
    # geometry: a tile that is enlarged in y (44 -> 50) and shrunk in x (52 -> 40), in a frame whose last word is partly
    # used (W = 77) and in one whose last word is full (W = 96)
    for W in (77, 96):
        H = 60
        for part, offs in zip("ab", _geometry(H, W, 50, 40)):
            for kind in ("random", "ones", "checker"):
                cases.append(PlaceCase(f"geometry_{part}_w{W}_{kind}", (44, 52), (50, 40), (H, W), tuple(offs), (kind,) * len(offs),
                                       telltale=(part == "a" and kind != "ones")))
    for W in (77, 96):      # H == 1: one frame row; the tile's rows 0 and 9 land on it, and one tile misses it
        cases.append(PlaceCase(f"one_row_frame_w{W}", (44, 52), (50, 40), (1, W), ((0, 0), (33, -9), (W - 1, 0), (5, 1), (W - 40, -49)),
                               _cycle(("random", "checker", "ones"), 5)))
    cases.append(PlaceCase("no_tiles", (44, 52), (50, 40), (60, 77), (), ()))
    return cases


PLACE_CASES = _place_cases()
PLACE_BY_NAME = {c.name: c for c in PLACE_CASES}
assert len(PLACE_BY_NAME) == len(PLACE_CASES)


def place_size_pairs():
    """Every (dst, src) pair of the table, for the three-way agreement of the index rule."""
    return sorted({p for c in PLACE_CASES for p in c.size_pairs()} | set(TELLTALE) | {(100, 70), (130, 91), (200, 140)})


# ------------------------------------------------------------------------------------------------------------------
# overlap removal and column counts: blobs
# ------------------------------------------------------------------------------------------------------------------
def blob(rng, H: int, W: int, max_h: int, max_w: int) -> np.ndarray:
    """A random ellipse with a tenth of its pixels knocked out."""
    h, w = int(rng.integers(3, max_h + 1)), int(rng.integers(3, max_w + 1))
    cy, cx = rng.uniform(0, H), rng.uniform(0, W)
    yy, xx = np.mgrid[0:H, 0:W]
    m = ((yy - cy) / (h / 2.0)) ** 2 + ((xx - cx) / (w / 2.0)) ** 2 <= 1.0
    return m & (rng.random((H, W)) > 0.1)


def tight_boxes(masks: np.ndarray) -> np.ndarray:
    return np.array([REF.area_bbox(m)[1] for m in masks], dtype=np.int32).reshape(len(masks), 4)


def grown_boxes(masks: np.ndarray, name: str, max_rows: int = 7, max_cols: int = 40) -> np.ndarray:
    """Supersets of the tight boxes: every side moved out by its own random amount (rows 0 .. 7, columns 0 .. 40), clipped to
    the frame; the box of an empty mask stays -1."""
    rng = _rng(name + "/grown")
    b = tight_boxes(masks).astype(np.int64)
    H, W = masks.shape[1:]
    for i in range(len(b)):
        if b[i, 0] < 0:
            continue
        b[i, 0] = max(b[i, 0] - int(rng.integers(0, max_rows + 1)), 0)
        b[i, 1] = max(b[i, 1] - int(rng.integers(0, max_cols + 1)), 0)
        b[i, 2] = min(b[i, 2] + int(rng.integers(0, max_rows + 1)), H - 1)
        b[i, 3] = min(b[i, 3] + int(rng.integers(0, max_cols + 1)), W - 1)
    return b.astype(np.int32)


@dataclass(frozen=True)
class OverlapCase:
    name: str
    frame: Tuple[int, int]
    lengths: Tuple[int, ...]              # masks per segment, in order
    use_seg: bool = True                  # False: seg = None (one segment)
    full_first: Optional[int] = None      # this segment starts with a full-frame mask: everything after it comes out empty

    @property
    def M(self) -> int:
        return sum(self.lengths)

    def seg(self) -> Optional[np.ndarray]:
        """Non-decreasing int32 ids with gaps (the kernels compare ids, they do not index with them)."""
        if not self.use_seg:
            return None
        ids = np.cumsum([1, 2, 1, 4, 1, 3, 2][:len(self.lengths)]) - 1
        return np.repeat(ids, self.lengths).astype(np.int32)

    def starts(self):
        return np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(int)


QUIET_ROWS = 3
FAR = ((256, 2), (257, 27), (512, 40), (513, 52))       # (distance, first column of the planted block; 27 .. 36 lies across a word boundary)


def far_pairs(s: int, n: int):
    """(h, m, x0) for a segment of n masks that starts at s: masks h < m that alone own a block of the frame's last
    ``QUIET_ROWS`` rows, where no blob reaches -- m can lose those pixels to h only, never to a mask in between.  Their
    distances are the ends of the box kernel's chunks of 256 earlier masks: 256 (the last mask of m's first chunk), 257 (the
    first of its second), 512 and 513.  A segment of 257 .. 262 masks has one pair: its first mask and the one 256 later,
    so that the chunk ends exactly where the segment starts."""
    out = [(s + 5 + k, s + 5 + k + d, x0) for k, (d, x0) in enumerate(FAR) if 5 + k + d < n - 2]
    if not out and n > 256:
        out = [(s, s + 256, FAR[0][1])]
    return out


@functools.lru_cache(maxsize=None)
def _overlap_masks(name: str) -> np.ndarray:
    c = OVERLAP_BY_NAME[name]
    rng = _rng(name)
    H, W = c.frame
    masks = np.stack([blob(rng, H, W, 24, 40) for _ in range(c.M)])
    masks[:, H - QUIET_ROWS:, :] = False                               # the quiet strip: only planted pixels live there
    for k, (s, n) in enumerate(zip(c.starts(), c.lengths)):
        if n >= 5:
            masks[s + n // 2] = False                                  # an empty mask (box -1) in the middle of the segment
            masks[s + n // 2 + 1] = masks[s + n // 2 - 1]              # identical to an earlier one: comes out empty
        if n >= 10:
            # two masks that touch at a word boundary and share no pixel: columns 20 .. 31 and 32 .. 45 of the same rows
            masks[s + 3] = False
            masks[s + 3, 4:20, 20:32] = True
            masks[s + 4] = False
            masks[s + 4, 4:20, 32:46] = True
        if n >= 260:
            masks[s + n - 2] = masks[s + 1]                            # identical to a mask more than one chunk of 256 earlier
        for h, m, x0 in far_pairs(int(s), int(n)):
            masks[h, H - QUIET_ROWS:, x0:x0 + 9] = True
            masks[m, H - QUIET_ROWS:, x0:x0 + 10] = True               # loses h's nine columns, keeps its own tenth
        if c.full_first == k:
            masks[s] = True
    masks.setflags(write=False)
    return masks


def overlap_masks(c: OverlapCase) -> np.ndarray:
    """bool [M, H, W], read-only."""
    return _overlap_masks(c.name)


@functools.lru_cache(maxsize=None)
def _overlap_want(name: str) -> np.ndarray:
    c = OVERLAP_BY_NAME[name]
    out = REF.overlap_prefix(overlap_masks(c), c.seg())
    out.setflags(write=False)
    return out


def overlap_want(c: OverlapCase) -> np.ndarray:
    return _overlap_want(c.name)


def chain_share(c: OverlapCase) -> float:
    """Share of the masks that lose a pixel which two or more earlier masks of their segment own (chains h < i < j < m)."""
    masks, seg = overlap_masks(c), c.seg()
    cover, hit = {}, 0
    for m in range(c.M):
        s = 0 if seg is None else int(seg[m])
        if s not in cover:
            cover[s] = np.zeros(c.frame, dtype=np.int64)
        hit += bool((masks[m] & (cover[s] >= 2)).any())
        cover[s] += masks[m]
    return hit / max(c.M, 1)


OVERLAP_CASES = [
    OverlapCase("four_of_10", (40, 70), (10, 10, 10, 10), full_first=2),
    OverlapCase("one_of_300", (40, 70), (300,)),
    OverlapCase("start_inside_a_chunk", (33, 64), (3, 300, 1, 530, 40), full_first=4),
    OverlapCase("around_256", (40, 70), (256, 257, 255)),
    OverlapCase("one_mask", (33, 64), (1,)),
    OverlapCase("no_seg_270", (40, 70), (270,), use_seg=False),
    OverlapCase("full_frame_first_of_270", (33, 64), (5, 270), full_first=1),
]
OVERLAP_BY_NAME = {c.name: c for c in OVERLAP_CASES}
BOX_MODES = ("tight", "grown", "none")
CHAIN_MIN_SEGMENT = 10          # the chain condition is asserted for cases whose longest segment has at least this many masks


def overlap_boxes(c: OverlapCase, mode: str) -> Optional[np.ndarray]:
    if mode == "none":
        return None
    return tight_boxes(overlap_masks(c)) if mode == "tight" else grown_boxes(overlap_masks(c), c.name)


# ------------------------------------------------------------------------------------------------------------------
# column counts
# ------------------------------------------------------------------------------------------------------------------
MIN_SIZES = (5, 25)             # the pipeline's thresholds: a column counts when its count is > min_size


@dataclass(frozen=True)
class CountCase:
    name: str
    frame: Tuple[int, int]
    use_seg: bool
    grown: bool

    @property
    def n_seg(self) -> int:
        return 6 if self.use_seg else 1


def threshold_columns(W: int):
    """(column, count) pairs on both sides of each threshold, at bit 3, at both sides of the first word boundary and in the
    frame's last column (four different columns at every width of the table)."""
    return ((3, 5), (31, 6), (32 if W > 33 else 30, 25), (W - 1, 26))


@functools.lru_cache(maxsize=None)
def _count_inputs(frame, use_seg):
    """(masks bool [M, H, W], seg int32 [M] or None).  With ``seg``: ids 0, 1, 3, 4 of 6 are used -- id 2 has no mask and id 5,
    the last, has none either.  Segment 0: blobs, one of them empty; segment 1: masks across columns 255/256 and 511/512
    where the frame has them, a mask in the last column, and 30 masks stacked on one column; segment 3: strips whose column
    counts are exactly 5, 6, 25 and 26; segment 4: more blobs, the last one empty."""
    H, W = frame
    rng = _rng(f"counts/{H}x{W}")
    groups = []
    g0 = [blob(rng, H, W, H, min(W, 60)) for _ in range(9)]
    g0[4] = np.zeros((H, W), dtype=bool)
    groups.append(g0)
    g1 = []
    for edge in (256, 512):
        if W > edge:
            m = np.zeros((H, W), dtype=bool)
            hi = min(edge + 2, W)
            m[1:H - 1, edge - 3:hi] = rng.random((H - 2, hi - edge + 3)) < 0.8
            m[2, edge - 1:edge + 1] = True
            g1.append(m)
    m = np.zeros((H, W), dtype=bool)
    m[:, W - 1] = True
    m[0, W - 2] = True
    g1.append(m)
    stack_col = min(W - 2, 40)
    for k in range(30):
        m = np.zeros((H, W), dtype=bool)
        m[:, stack_col] = True
        m[k % H, max(stack_col - 1 - k % 3, 0)] = True
        g1.append(m)
    groups.append(g1)
    g3 = []
    for col, n in threshold_columns(W):
        left = n
        while left > 0:
            m = np.zeros((H, W), dtype=bool)
            rows = min(left, H)
            y0 = int(rng.integers(0, H - rows + 1))
            m[y0:y0 + rows, col] = True
            g3.append(m)
            left -= rows
    groups.append(g3)
    g4 = [blob(rng, H, W, H, min(W, 90)) for _ in range(6)] + [np.zeros((H, W), dtype=bool)]
    groups.append(g4)
    masks = np.stack([m for g in groups for m in g])
    seg = np.repeat(np.array([0, 1, 3, 4], dtype=np.int32), [len(g) for g in groups]) if use_seg else None
    masks.setflags(write=False)
    if seg is not None:
        seg.setflags(write=False)
    return masks, seg


def count_inputs(c: CountCase):
    return _count_inputs(c.frame, c.use_seg)


def count_boxes(c: CountCase) -> np.ndarray:
    masks, _ = count_inputs(c)
    return grown_boxes(masks, c.name) if c.grown else tight_boxes(masks)


COUNT_FRAMES = ((20, 33), (40, 70), (12, 300), (9, 513))
COUNT_CASES = [CountCase(f"{h}x{w}_{'seg' if s else 'noseg'}_{'grown' if g else 'tight'}", (h, w), s, g)
               for (h, w) in COUNT_FRAMES for s in (True, False) for g in (False, True)]
COUNT_BY_NAME = {c.name: c for c in COUNT_CASES}
