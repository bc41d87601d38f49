"""Dense reference of the error maps (``demia_mask_error_map`` / ``demia_crop_error_map``): the definitions of
``include/deepemia_hip.h`` restated on boolean images with NumPy and SciPy, independent of the kernel's words, tiles and rounds.

    unions      boolean ORs of the masks of a state
    outline     m & ~binary_erosion(m, ones((2t + 1, 2t + 1)), border_value=0)
    blend       (b * (256 - alpha) + colour * alpha + 128) >> 8 in integers
    priority    lines over fills; unmatched detection > missed annotation > matched detection > matched annotation > crowd region
    counts      agree, excess, missing, ignored: of the fill classes, whatever the lines cover
"""
from typing import Sequence, Tuple

import numpy as np
from scipy import ndimage

# BGR, stated here on its own: agree, excess, missing, then the five line classes by priority
PALETTE = np.array([[0, 255, 0], [0, 0, 255], [255, 0, 0], [255, 0, 255], [255, 255, 0], [0, 255, 255], [255, 255, 255], [128, 128, 128]],
                   dtype=np.uint8)


def union(masks: np.ndarray, states: Sequence[int], wanted: Tuple[int, ...], hw: Tuple[int, int]) -> np.ndarray:
    out = np.zeros(hw, dtype=bool)
    for m, s in zip(masks, states):
        if int(s) in wanted:
            out |= m.astype(bool)
    return out


def outline(mask: np.ndarray, t: int) -> np.ndarray:
    m = mask.astype(bool)
    if not m.any():
        return m.copy()
    return m & ~ndimage.binary_erosion(m, structure=np.ones((2 * t + 1, 2 * t + 1), dtype=bool), border_value=0)


def fill_classes(det, d_state, gt, g_state, hw):
    """(agree, ignored, excess, missing) boolean images."""
    dall, gall, gc = union(det, d_state, (1, 2), hw), union(gt, g_state, (1, 2), hw), union(gt, g_state, (3,), hw)
    agree = dall & gall
    ignored = dall & gc & ~gall
    excess = dall & ~gall & ~gc
    missing = gall & ~dall
    return agree, ignored, excess, missing


def line_classes(det, d_state, gt, g_state, t, hw):
    """The five line classes in priority order: boolean images of the outlines of the masks of each state."""
    def lines(masks, states, wanted):
        out = np.zeros(hw, dtype=bool)
        for m, s in zip(masks, states):
            if int(s) == wanted:
                out |= outline(m, t)
        return out
    return [lines(det, d_state, 2), lines(gt, g_state, 2), lines(det, d_state, 1), lines(gt, g_state, 1), lines(gt, g_state, 3)]


def base_image(src: np.ndarray) -> np.ndarray:
    src = np.asarray(src, dtype=np.uint8)
    if src.ndim == 2:
        src = src[:, :, None]
    return np.repeat(src, 3, axis=2) if src.shape[2] == 1 else src.copy()


def error_map(det: np.ndarray, d_state, gt: np.ndarray, g_state, src: np.ndarray, alpha: int, t: int, palette=None
              ) -> Tuple[np.ndarray, np.ndarray]:
    """``det`` [D, H, W] / ``gt`` [G, H, W] boolean, ``src`` [H, W] / [H, W, 1] / [H, W, 3] uint8: (dst [H, W, 3] uint8, counts [4] int64 =
    agree, excess, missing, ignored)."""
    pal = (PALETTE if palette is None else np.asarray(palette)).astype(np.int64).reshape(8, 3)
    b = base_image(src)
    hw = b.shape[:2]
    agree, ignored, excess, missing = fill_classes(det, d_state, gt, g_state, hw)
    out = b.astype(np.int64)
    for k, cls in enumerate((agree, excess, missing)):
        out[cls] = (out[cls] * (256 - int(alpha)) + pal[k] * int(alpha) + 128) >> 8
    for k, cls in reversed(list(enumerate(line_classes(det, d_state, gt, g_state, int(t), hw)))):      # the highest class is painted last
        out[cls] = pal[3 + k]
    counts = np.array([agree.sum(), excess.sum(), missing.sum(), ignored.sum()], dtype=np.int64)
    return out.astype(np.uint8), counts
