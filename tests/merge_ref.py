"""Independent dense references of the tile-merge stages (``place_tile_kernel``, ``crop_place_kernel``,
``overlap_prefix*_kernel``, ``column_counts_kernel``) in plain Python and numpy: bool planes and int64 counts, no packed
words in any computation.  Nothing here imports the package, the oracle or ``cropset.nearest_index``; ``test_cpu_merge_ref.py``
checks these references against those writings and against their own properties.

  * ``nearest_rule``: cv2's INTER_NEAREST source index in float64, a scalar loop; ``rule_integer``, ``rule_direct_ratio`` and
    ``rule_f32`` are three plausible WRONG writings of it, kept so that the case table can prove it tells them apart;
  * ``place``: resize by a rule, paste at an offset (negative allowed), clip to the frame;
  * ``overlap_prefix``: score-ordered overlap removal, one ``seen`` plane per segment;
  * ``column_counts``: pixels per column and segment;
  * ``area_bbox``: pixel count and tight box (y0, x0, y1, x1), -1 when empty;
  * ``pack`` / ``unpack``: dense <-> ``[M, H, ceil(W / 32)]`` words, pixel x = bit ``x & 31`` of word ``x >> 5``.
"""
import math

import numpy as np


# ------------------------------------------------------------------------------------------------------------ index rules
def nearest_rule(n_dst: int, n_src: int) -> np.ndarray:
    """``min(floor(t * (1 / (n_dst / n_src))), n_src - 1)`` for t = 0 .. n_dst - 1; Python floats are IEEE doubles."""
    out = np.empty(n_dst, dtype=np.int64)
    for t in range(n_dst):
        out[t] = min(math.floor(t * (1.0 / (n_dst / n_src))), n_src - 1)
    return out


def rule_integer(n_dst: int, n_src: int) -> np.ndarray:
    """WRONG on purpose: exact integer arithmetic."""
    return np.array([min(t * n_src // n_dst, n_src - 1) for t in range(n_dst)], dtype=np.int64).reshape(n_dst)


def rule_direct_ratio(n_dst: int, n_src: int) -> np.ndarray:
    """WRONG on purpose: the factor taken as ``n_src / n_dst`` in one division, not as the reciprocal of ``n_dst / n_src``."""
    return np.array([min(math.floor(t * (n_src / n_dst)), n_src - 1) for t in range(n_dst)], dtype=np.int64).reshape(n_dst)


def rule_f32(n_dst: int, n_src: int) -> np.ndarray:
    """WRONG on purpose: the rule's own expression, every operation in float32."""
    f = np.float32
    fac = f(1.0) / (f(n_dst) / f(n_src))
    assert fac.dtype == np.float32
    return np.array([min(int(np.floor(f(t) * fac)), n_src - 1) for t in range(n_dst)], dtype=np.int64).reshape(n_dst)


WRONG_RULES = {"integer": rule_integer, "direct_ratio": rule_direct_ratio, "f32": rule_f32}


# -------------------------------------------------------------------------------------------------------------- placement
def place(src_dense, tile_h: int, tile_w: int, xo: int, yo: int, H: int, W: int, rule=nearest_rule) -> np.ndarray:
    """bool [H, W]: ``src_dense`` [sh, sw] resized to (tile_h, tile_w) by ``rule`` on each axis, its pixel (0, 0) put at
    column ``xo`` and row ``yo`` of a zero frame, whatever falls outside the frame dropped."""
    src = np.asarray(src_dense, dtype=bool)
    sh, sw = src.shape
    iy, ix = rule(tile_h, sh), rule(tile_w, sw)
    out = np.zeros((H, W), dtype=bool)
    rows = [(ty + yo, int(iy[ty])) for ty in range(tile_h) if 0 <= ty + yo < H]            # (frame row, source row)
    cols = [(tx + xo, int(ix[tx])) for tx in range(tile_w) if 0 <= tx + xo < W]
    if rows and cols:
        out[np.ix_([r[0] for r in rows], [c[0] for c in cols])] = src[np.ix_([r[1] for r in rows], [c[1] for c in cols])]
    return out


# ---------------------------------------------------------------------------------------------------------------- overlap
def overlap_prefix(masks, seg=None) -> np.ndarray:
    """bool [M, H, W]: mask m without every pixel that an earlier mask of its segment has (``seg`` None: one segment)."""
    masks = np.asarray(masks, dtype=bool)
    out = np.zeros_like(masks)
    seen = {}
    for m in range(masks.shape[0]):
        s = 0 if seg is None else int(seg[m])
        if s not in seen:
            seen[s] = np.zeros(masks.shape[1:], dtype=bool)
        out[m] = masks[m] & ~seen[s]
        seen[s] |= masks[m]
    return out


def column_counts(masks, seg, n_seg: int) -> np.ndarray:
    """int64 [n_seg, W]: set pixels per column, summed over the masks of each segment (``seg`` None: all in row 0)."""
    masks = np.asarray(masks, dtype=bool)
    out = np.zeros((n_seg, masks.shape[2]), dtype=np.int64)
    for m in range(masks.shape[0]):
        out[0 if seg is None else int(seg[m])] += masks[m].sum(axis=0, dtype=np.int64)
    return out


def area_bbox(mask):
    """(pixel count, [y0, x0, y1, x1] inclusive; all -1 for an empty mask)."""
    ys, xs = np.nonzero(np.asarray(mask, dtype=bool))
    if ys.size == 0:
        return 0, [-1, -1, -1, -1]
    return int(ys.size), [int(ys.min()), int(xs.min()), int(ys.max()), int(xs.max())]


# ----------------------------------------------------------------------------------------------------------- packed words
def pack(dense, W: int, pad_ones: bool = False) -> np.ndarray:
    """bool [..., H, W] -> uint32 [..., H, ceil(W / 32)].  ``pad_ones``: the unused high bits of each row's last word are set
    (what a kernel must never read as pixels); else they are 0."""
    dense = np.asarray(dense, dtype=bool)
    assert dense.shape[-1] == W
    wpr = (W + 31) // 32
    bits = np.full(dense.shape[:-1] + (wpr * 32,), bool(pad_ones), dtype=bool)
    bits[..., :W] = dense
    weights = np.uint64(1) << np.arange(32, dtype=np.uint64)
    words = (bits.reshape(dense.shape[:-1] + (wpr, 32)).astype(np.uint64) * weights).sum(axis=-1, dtype=np.uint64)
    return words.astype(np.uint32)


def unpack(words, W: int):
    """uint32 [..., H, wpr] -> (bool [..., H, W], bool [..., H, 32 * wpr - W]: the padding bits)."""
    words = np.asarray(words).astype(np.uint32)
    wpr = words.shape[-1]
    assert wpr == (W + 31) // 32
    bits = ((words[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).astype(bool)
    bits = bits.reshape(words.shape[:-1] + (wpr * 32,))
    return bits[..., :W], bits[..., W:]
