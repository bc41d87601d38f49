"""The calls the mask paste is tested on (``test_cpu_paste_ref.py``, ``test_gpu_paste_edges.py``): a table of small named
CASES, each ONE call of ``demia_paste_masks`` -- a frame, N images of D slots, a count per image, and per slot a named box,
a 28 x 28 mask and a class.  What a slot is there for is in its name and in ``expect`` (validity, which column path of the
kernel its window width selects); the CPU test checks every expectation, so that a case cannot quietly stop reaching its
branch.  Slots at and beyond ``count`` hold decoys: a valid box over most of the frame with an all-ones mask, which fills
the plane if it is ever read.

Frames (img_h, img_w -> out_h, out_w).  Widths 32, 33, 77, 128, 333 and 2300; heights that are and are not multiples of the
kernel's 16-row chunk; words per row (wpr) with wpr % 4 zero (the 16-byte zero stores) and non-zero; two rescaling frames
with unequal, non-dyadic x and y ratios.  The wide frame is the only one above ``PASTE_COLS`` = 2048 columns: there the
kernel leaves its per-column LDS table for the per-pixel path, by the WINDOW width ``x1i - x0i``.

``reference(case)`` is the f64 reference of a case, computed once per process and read-only.

The tie band.  A pixel whose f64 probability lies within ``TAU`` = 2^-14 of 0.5 is ambiguous (either decision is accepted
from an f32 implementation); the derivation is in ``test_gpu_paste_edges.py``.  ``MAX_AMBIGUOUS_SHARE``: ambiguous pixels
may be at most 0.5 % of the window pixels of the table (the EXACT family aside, which has no band at all).
"""
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

import paste_ref as REF

TAU = 2.0 ** -14
MAX_AMBIGUOUS_SHARE = 0.005
PASTE_COLS = 2048            # csrc/paste.hip: the widest window whose column table fits the workgroup's LDS
PASTE_ROWS = 16              # csrc/paste.hip: rows per block of the whole-plane paste
D_SMALL, D_WIDE = 32, 100


@dataclass(frozen=True)
class Frame:
    name: str
    img_h: int
    img_w: int
    out_h: int
    out_w: int

    @property
    def wpr(self) -> int:
        return (self.out_w + 31) // 32

    @property
    def rescales(self) -> bool:
        return (self.img_h, self.img_w) != (self.out_h, self.out_w)


FRAMES = {f.name: f for f in (
    Frame("w32", 32, 32, 32, 32),                # one word per row, H a multiple of 16
    Frame("w33", 23, 33, 23, 33),                # one pixel in the second word
    Frame("w77", 50, 77, 50, 77),                # wpr 3
    Frame("w128", 48, 128, 48, 128),             # wpr 4: whole rows of zeros go out as 16-byte stores
    Frame("w128_h45", 45, 128, 45, 128),         # the same with a short last chunk
    Frame("w333", 60, 333, 60, 333),             # wpr 11, a short last chunk
    Frame("wide", 40, 2300, 40, 2300),           # wpr 72: windows wider than PASTE_COLS
    Frame("down_800_333", 600, 800, 200, 333),   # x 0.41625, y 1/3
    Frame("up_97_291", 64, 97, 100, 291),        # x 3, y 1.5625
)}


@dataclass
class Slot:
    name: str
    box: Tuple[float, float, float, float]       # x0, y0, x1, y1 in the network's frame (img_h x img_w)
    mask: np.ndarray                             # [28, 28] float32
    cls: int
    expect: Dict[str, object] = field(default_factory=dict)      # valid: bool; path: "table" | "pixel"


@dataclass
class Case:
    name: str
    frame: Frame
    K: int
    D: int
    counts: List[int]
    slots: List[List[Slot]]                      # [N][D]
    exact: bool = False                          # every f32 operation of the kernel is exact on it: no tie band

    @property
    def N(self) -> int:
        return len(self.slots)

    def det_boxes(self) -> np.ndarray:
        return np.array([[s.box for s in img] for img in self.slots], dtype=np.float32)

    def masks(self) -> np.ndarray:
        return np.stack([np.stack([s.mask for s in img]) for img in self.slots]).astype(np.float32)

    def classes(self) -> np.ndarray:
        return np.array([[s.cls for s in img] for img in self.slots], dtype=np.int32)

    def mask_prob(self) -> np.ndarray:
        return REF.blocked_mask_prob(self.masks().reshape(-1, 28, 28), self.classes().reshape(-1), self.K)

    def used(self):
        """(n, i, slot) of every slot below its image's count."""
        return [(n, i, self.slots[n][i]) for n in range(self.N) for i in range(self.counts[n])]


# ------------------------------------------------------------------------------------------------------------------
# masks
# ------------------------------------------------------------------------------------------------------------------
def blob(rng) -> np.ndarray:
    """A smooth bump: above 0.5 in a disc of the box's middle, below it towards the rim."""
    yy, xx = np.meshgrid(np.arange(28.0), np.arange(28.0), indexing="ij")
    cy, cx = rng.uniform(11.0, 16.0, size=2)
    sig = rng.uniform(5.0, 9.0)
    return np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * sig * sig)).astype(np.float32)


def binary(rng) -> np.ndarray:
    """Random 0 / 1 cells: slope 1 per cell, where a tap or a weight that is off by one column shows on many pixels."""
    return (rng.random((28, 28)) < 0.5).astype(np.float32)


def uniform(rng) -> np.ndarray:
    return rng.random((28, 28)).astype(np.float32)


def quarters(rng) -> np.ndarray:
    """Multiples of 1/4 in 0 .. 1 (the exact family)."""
    return (rng.integers(0, 5, size=(28, 28)) * 0.25).astype(np.float32)


def ones(rng=None) -> np.ndarray:
    return np.ones((28, 28), dtype=np.float32)


MASK_KINDS = (blob, binary, uniform)


# ------------------------------------------------------------------------------------------------------------------
# boxes
# ------------------------------------------------------------------------------------------------------------------
INVALID, VALID = dict(valid=False), dict(valid=True)


def geometry(H: int, W: int):
    """(name, box, expect) of the degenerate and edge geometry on an H x W frame that is not rescaled (H >= 23, W >= 32)."""
    g = [
        ("outside_left", (-30.0, 3.0, -5.0, H - 3.0), INVALID),
        ("outside_right", (W + 3.0, 3.0, W + 20.5, H - 3.0), INVALID),
        ("outside_top", (3.0, -40.5, W - 3.0, -2.0), INVALID),
        ("outside_bottom", (3.0, H + 0.5, W - 3.0, H + 30.0), INVALID),
        ("clipped_to_zero_width_at_0", (-10.0, 2.0, 0.0, H - 2.0), INVALID),
        ("clipped_to_zero_height_at_H", (2.0, float(H), W - 2.0, H + 9.0), INVALID),
        ("zero_width_inside", (12.5, 4.0, 12.5, 18.0), INVALID),
        ("negative_width", (20.0, 5.0, 10.0, 15.0), INVALID),
        ("sliver_0p3_px", (10.35, 2.5, 10.65, H - 2.5), VALID),
        ("inside_one_word", (3.3, 4.2, 20.7, H - 4.6), VALID),
        ("integer_corners", (4.0, 3.0, 20.0, 19.0), VALID),
        ("half_integer_corners", (4.5, 3.5, 20.5, 19.5), VALID),
        ("whole_frame", (0.0, 0.0, float(W), float(H)), VALID),
        ("beyond_the_frame", (-5.5, -7.25, W + 5.5, H + 3.0), VALID),
        ("far_out_of_range", (-1e30, -1e30, 1e30, 1e30), VALID),
        ("far_negative_corner", (-1e6, -2e9, 7.5, 9.25), VALID),
        ("clipped_at_right_edge", (W - 10.3, 5.5, W + 4.0, H - 1.5), VALID),
        ("clipped_at_bottom_left", (-3.7, H - 9.4, 12.2, H + 100.0), VALID),
        ("one_pixel_at_the_last_corner", (W - 1.0, H - 1.0, float(W), float(H)), VALID),
    ]
    if W >= 42:
        g.append(("across_a_word_boundary", (25.5, 2.25, 40.25, H - 3.5), VALID))
    first_of_last_word = 32 * ((W - 1) // 32)
    if first_of_last_word >= 32:
        g.append(("across_into_the_last_word", (first_of_last_word - 5.5, 3.75, W - 0.75, H - 2.25), VALID))
    return g


def wide_paths(H: int, W: int):
    """The boxes of the wide frame that sit on the limit between the two column paths (the window is two to three columns
    wider than the box: floor - 1 .. ceil + 1)."""
    return [
        ("table_window_1803", (100.5, 3.5, 1900.25, H - 3.75), dict(valid=True, path="table", ncol=1803)),
        ("table_window_2048", (101.5, 2.25, 2146.5, H - 5.5), dict(valid=True, path="table", ncol=2048)),
        ("table_window_2048_clipped_left", (-50.0, 4.0, 2046.2, H - 4.0), dict(valid=True, path="table", ncol=2048)),
        ("pixel_window_2049", (101.5, 2.25, 2147.5, H - 5.5), dict(valid=True, path="pixel", ncol=2049)),
        ("pixel_window_2101_to_the_right_edge", (200.3, 1.5, W - 0.3, H - 1.25), dict(valid=True, path="pixel", ncol=2101)),
        ("pixel_full_width", (0.0, 0.0, float(W), float(H)), dict(valid=True, path="pixel", ncol=W)),
        ("pixel_far_out_of_range", (-1e30, 5.0, 1e30, H - 6.5), dict(valid=True, path="pixel", ncol=W)),
        ("pixel_2200_px_wide_0p4_px_high", (50.25, 20.3, 2250.75, 20.7), dict(valid=True, path="pixel")),
    ]


def random_boxes(rng, n: int, H: int, W: int):
    """Boxes of every size from 1.5 px to most of the frame with their centres inside it, so that up to half of a box hangs
    over an edge (H, W: the network's frame)."""
    out = []
    for k in range(n):
        cx, cy = rng.uniform(0.0, W), rng.uniform(0.0, H)
        w = 1.5 + rng.random() ** 2 * 0.9 * W
        h = 1.5 + rng.random() ** 2 * 0.9 * H
        out.append((f"random_{k}", (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), {}))
    return out


def _decoy(frame: Frame) -> Slot:
    return Slot("decoy", (1.0, 1.0, frame.img_w - 1.0, frame.img_h - 1.0), ones(), 0)


def _image(frame: Frame, named, rng, K: int, D: int, mask_of=None) -> List[Slot]:
    slots = []
    for k, (name, box, expect) in enumerate(named):
        m = mask_of(k, rng) if mask_of else MASK_KINDS[k % 3](rng)
        slots.append(Slot(name, tuple(float(v) for v in box), m, int(rng.integers(0, K)), dict(expect)))
    assert len(slots) <= D, (len(slots), D)
    return slots + [_decoy(frame) for _ in range(D - len(slots))]


def _build():
    cases = []
    for fi, f in enumerate(FRAMES.values()):
        D = D_WIDE if f.name == "wide" else D_SMALL
        K = (1, 2, 3, 5)[fi % 4]
        rng = np.random.default_rng(1000 + fi)
        H, W = f.img_h, f.img_w
        if not f.rescales:
            # every edge of the geometry; the second image holds the same boxes in reverse order and uses ONE of them
            g = geometry(H, W) + (wide_paths(H, W) if f.name == "wide" else [])
            named = {name: (name, box, expect) for name, box, expect in g}
            cases.append(Case(f"geom_{f.name}", f, K, D, [len(g), 1],
                              [_image(f, g, rng, K, D), _image(f, [named["whole_frame"]] + g[::-1], rng, K, D)]))
            # every slot in use in one image (count = D), a few in the other
            cases.append(Case(f"rand_{f.name}", f, K, D, [7, D],
                              [_image(f, random_boxes(rng, D, H, W), rng, K, D), _image(f, random_boxes(rng, D, H, W), rng, K, D)]))
            # almost nothing left: two invalid boxes and a small valid one, then an image with count = 0
            few = [named["outside_left"], named["clipped_to_zero_width_at_0"], ("small", (W - 20.25, 6.5, W - 7.5, 17.75), VALID)]
            cases.append(Case(f"gone_{f.name}", f, K, D, [3, 0],
                              [_image(f, few, rng, K, D), _image(f, random_boxes(rng, 5, H, W), rng, K, D)]))
        else:
            edges = [
                ("whole_image", (0.0, 0.0, float(W), float(H)), VALID),
                ("beyond_the_image", (-9.5, -3.25, W + 7.0, H + 11.5), VALID),
                ("outside_right", (W + 0.5, 5.0, W + 40.0, H - 5.0), INVALID),
                ("outside_bottom", (5.0, H + 0.25, W - 5.0, H + 40.0), INVALID),
                ("clipped_to_zero_width_at_0", (-12.0, 5.0, 0.0, H - 5.0), INVALID),
                ("far_out_of_range", (-1e30, -1e30, 1e30, 1e30), VALID),
                ("thin_after_scaling", (0.3 * W + 0.6, 0.2 * H, 0.3 * W + 1.8, 0.8 * H), VALID),
            ]
            cases.append(Case(f"rescale_{f.name}", f, K, D, [D, 5],
                              [_image(f, edges + random_boxes(rng, D - len(edges), H, W), rng, K, D),
                               _image(f, random_boxes(rng, 9, H, W), rng, K, D)]))
    cases.append(_exact_case())
    return cases


# The exact family: widths and heights that are powers of two, corners on multiples of 1/4 inside the frame (so the clip
# changes nothing), no rescaling, mask values multiples of 1/4.  Then X + 0.5 - x0 is a multiple of 1/4 below 2^8, its
# quotient by the width a multiple of 2^-9, the cell coordinate a multiple of 2^-7 below 2^6, each weight a multiple of
# 2^-7 in [0, 1], each product of two weights and a mask value a multiple of 2^-16 in [0, 1], and so is every partial sum:
# every f32 operation of the kernel (and of any other f32 implementation of the same formula) is exact, and the f32 result
# IS the f64 one.  No tie band applies.  A half-integer x0 under an all-ones mask puts pixel centres exactly on the box's
# edge, where the probability is exactly 0.5: the family pins `>=`.
EXACT_FRAME = Frame("exact_150x200", 150, 200, 150, 200)
EXACT_BOXES = (
    # x0, y0, width, height, mask
    (4.5, 3.5, 16, 16, ones),
    (10.25, 20.75, 32, 16, quarters),
    (0.0, 0.0, 128, 128, quarters),
    (72.0, 22.0, 128, 128, ones),
    (50.5, 60.5, 64, 32, binary),
    (100.75, 5.25, 64, 64, quarters),
    (20.5, 100.5, 32, 32, ones),
    (150.0, 10.0, 16, 128, binary),
    (33.5, 40.0, 128, 64, ones),
    (31.5, 15.5, 32, 128, quarters),
    (95.75, 63.5, 64, 16, binary),
    (160.5, 130.25, 16, 16, quarters),
)


def _exact_case() -> Case:
    f = EXACT_FRAME
    rng = np.random.default_rng(77)
    named = [(f"exact_{w}x{h}_at_{x0}_{y0}_{m.__name__}", (x0, y0, x0 + w, y0 + h), VALID) for (x0, y0, w, h, m) in EXACT_BOXES]
    img = _image(f, named, rng, 2, D_SMALL, mask_of=lambda k, r: EXACT_BOXES[k][4](r))
    return Case("exact_family", f, 2, D_SMALL, [len(named)], [img], exact=True)


CASES: List[Case] = _build()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# Three successive pastes into the same planes (same frame, N and D): boxes that move, a round in which every slot is in use,
# and a round in which almost every instance is gone or invalid -- in both orders.
INCREMENTAL = {
    "w333": ("geom_w333", "rand_w333", "gone_w333"),
    "w128": ("rand_w128", "gone_w128", "geom_w128"),
    "w33": ("gone_w33", "geom_w33", "rand_w33"),
    "wide": ("geom_wide", "gone_wide", "rand_wide"),
}


# ------------------------------------------------------------------------------------------------------------------
# the reference of a case, once
# ------------------------------------------------------------------------------------------------------------------
@dataclass
class Reference:
    out_boxes: np.ndarray                         # [N, D, 4] float32: zero at and beyond count
    valid: np.ndarray                             # [N, D] bool
    hint: np.ndarray                              # [N, D, 4] int32: y0, x0, y1, x1 inclusive; -1 where nothing is pasted
    prob: Dict[Tuple[int, int], np.ndarray]       # (n, i) of every valid slot -> float64 [window rows, window columns]


_REFS: Dict[str, Reference] = {}


def reference(case: Case) -> Reference:
    if case.name not in _REFS:
        f = case.frame
        ob, valid = REF.out_boxes(case.det_boxes(), f.img_h, f.img_w, f.out_h, f.out_w)
        hint = np.full((case.N, case.D, 4), -1, dtype=np.int32)
        prob = {}
        masks = case.masks()
        for n in range(case.N):
            ob[n, case.counts[n]:] = 0.0
            valid[n, case.counts[n]:] = False
            for i in np.nonzero(valid[n])[0]:
                plane, win = REF.paste64(masks[n, i], ob[n, i], f.out_h, f.out_w)
                hint[n, i] = REF.hint_of(win)
                p = np.ascontiguousarray(plane[win[0]:win[2], win[1]:win[3]])
                p.setflags(write=False)
                prob[(n, int(i))] = p
        for a in (ob, valid, hint):
            a.setflags(write=False)
        _REFS[case.name] = Reference(ob, valid, hint, prob)
    return _REFS[case.name]


def decided(case: Case, p: np.ndarray) -> np.ndarray:
    """The pixels of a probability window on which an f32 implementation has to agree with the f64 decision."""
    return np.ones(p.shape, dtype=bool) if case.exact else np.abs(p - 0.5) > TAU


def pixel_centres(box_f32):
    """How many pixel centres (k + 0.5) the closed f32 box holds on x and on y."""
    x0, y0, x1, y1 = (float(v) for v in box_f32)
    return (int(np.floor(x1 - 0.5) - np.ceil(x0 - 0.5)) + 1, int(np.floor(y1 - 0.5) - np.ceil(y0 - 0.5)) + 1)


def needs_both_values(slot: Slot, box_f32) -> bool:
    """Whether the slot's window must hold decided pixels of both values.  Every named slot must; a random box only when it
    is not degenerate, that is when it holds at least three pixel centres on each axis (a box under two pixels samples its
    mask at one or two points a row, each diluted by the zero padding: whether any reaches 0.5 is up to the mask)."""
    return not slot.name.startswith("random_") or min(pixel_centres(box_f32)) >= 3


def column_path(hint_row) -> str:
    """Which column path of the kernel a window of this width takes."""
    return "table" if int(hint_row[3]) - int(hint_row[1]) + 1 <= PASTE_COLS else "pixel"
