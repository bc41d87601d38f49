"""References for the image front end (``csrc/preproc_stem.hip``): what ``test_gpu_front_end_edges.py`` holds the kernels to.

  * Pillow itself for the resize (``pillow_reference``), and a NumPy replay of Pillow's two integer passes from
    ``engine.pil_bilinear_tables`` (``pillow_replay``) that the CPU test compares with Pillow: the tables are then not the
    suspect when a kernel test fails.
  * ``cv_linear_u8``: a per-pixel scalar restatement of OpenCV's 8-bit ``INTER_LINEAR`` resize.  It computes its own
    coefficients and shares no code with ``engine.cv_linear_tables`` or ``oracle/pipeline_ref.py``.
  * float64 convolution and max pool for the stem, and a torch restatement of the P32 plane split for the pool.

Every reference takes the name of ONE deliberate mistake (``front_end_cases.VARIANTS``); the CPU test shows that each moves the
result past the pass rule of the GPU test.

Distance of the fixed-point linear resize from exact bilinear interpolation (``LINEAR_BOUND``), in grey levels
---------------------------------------------------------------------------------------------------------------------
Let w be an exact weight, c = rint(2048 w~) its 11-bit coefficient, where w~ is w computed in f32.  The coordinate
``(d + 0.5) * scale - 0.5`` is rounded to f32 once (relative 2^-24 of a value below ``LINEAR_MAX_EXTENT`` = 128), ``f - floor(f)``
is exact, ``1 - f`` rounds once more (2^-25): |w~ - w| <= 128 * 2^-24 + 2^-25 =: d, so |c / 2048 - w| <= E = (0.5 + 2048 d) / 2048.

  horizontal: h = S0 c0 + S1 c1 exactly; |h / 2048 - (S0 w0 + S1 w1)| <= 2 * 255 * E.
  ``r = h >> 4`` loses t1 in [0, 15/16]:  r = 128 (h / 2048) - t1.
  vertical, per row j: ``(b_j r_j) >> 16`` = 4 B_j (h_j / 2048) - B_j t1 / 32 - t2 with B_j = b_j / 2048 and t2 in [0, 1).
  Their sum is X = 4 V - tau, V = sum_j B_j (h_j / 2048), 0 <= tau < 2 + (B_0 + B_1) * (15/16) / 32 <= 2 + (1 + 2 E) * 15 / 512.
  ``v = (X + 2) >> 2`` = floor(V + 0.5 - tau / 4), so  V - 0.5 - tau / 4 < v <= V + 0.5:  |v - V| < 0.5 + tau_max / 4.
  V against exact bilinear: the horizontal error through weights that sum to at most 1 + 2 E, plus the vertical coefficients'
  own 2 * 255 * E:  |V - exact| <= 510 E (1 + 2 E) + 510 E.
  Clipping to [0, 255] never increases the distance (the exact value lies inside).

  LINEAR_BOUND = 0.5 + (2 + (1 + 2 E) * 15 / 512) / 4 + 510 E (2 + 2 E) = 1.264 grey levels.

The replicated border of the exact interpolation is what both OpenCV edge rules mean in exact arithmetic: horizontally the
index is clamped and the fraction zeroed (all weight on the border pixel), vertically the fraction is kept and both ROWS are
clipped onto the border row (the two weights land on the same pixel).  In fixed point the second form truncates twice, which
is how the two rules come to differ in a byte (``front_end_cases.EDGE_RULE_CASE``).
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn.functional as F

import front_end_cases as S

MEAN32 = np.array(S.PIXEL_MEAN, dtype=np.float32)

_D = S.LINEAR_MAX_EXTENT * 2.0 ** -24 + 2.0 ** -25
_E = (0.5 + 2048.0 * _D) / 2048.0
LINEAR_BOUND = 0.5 + (2.0 + (1.0 + 2.0 * _E) * 15.0 / 512.0) / 4.0 + 510.0 * _E * (2.0 + 2.0 * _E)


# ---------------------------------------------------------------------------------------------------------------------
# Pillow
# ---------------------------------------------------------------------------------------------------------------------
def pillow_resize_u8(imgs: np.ndarray, new_h: int, new_w: int) -> np.ndarray:
    from PIL import Image
    return np.stack([np.asarray(Image.fromarray(im).resize((new_w, new_h), Image.BILINEAR)) for im in imgs])


def pillow_reference(imgs: np.ndarray, new_h: int, new_w: int) -> np.ndarray:
    """[n, new_h, new_w, 3] f32: ``Image.resize((new_w, new_h), Image.BILINEAR)`` minus PIXEL_MEAN."""
    return pillow_resize_u8(imgs, new_h, new_w).astype(np.float32) - MEAN32


def _pillow_pass(a: np.ndarray, axis: int, out_size: int, rounding: int) -> np.ndarray:
    from deepemia_amd.engine import pil_bilinear_tables
    lo, cnt, k = pil_bilinear_tables(a.shape[axis], out_size)
    a = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + a.shape[1:], dtype=np.int64)
    for o in range(out_size):
        kk = k[o, :cnt[o]].astype(np.int64).reshape((-1,) + (1,) * (a.ndim - 1))
        out[o] = rounding + (a[lo[o]:lo[o] + cnt[o]] * kk).sum(axis=0)
    return np.moveaxis(np.clip(out >> 22, 0, 255).astype(np.uint8), 0, axis)


def pillow_replay(imgs: np.ndarray, new_h: int, new_w: int, variant: Optional[str] = None) -> np.ndarray:
    """Pillow's two 8-bit passes (horizontal first, u8 in between) from the host tables, in NumPy: [n, new_h, new_w, 3] u8.
    A pass whose size does not change is skipped, as Pillow skips it."""
    assert variant in (None, "pillow_no_rounding"), variant
    rounding = 0 if variant == "pillow_no_rounding" else 1 << 21
    a = imgs
    if new_w != a.shape[2]:
        a = _pillow_pass(a, 2, new_w, rounding)
    if new_h != a.shape[1]:
        a = _pillow_pass(a, 1, new_h, rounding)
    return a


# ---------------------------------------------------------------------------------------------------------------------
# OpenCV INTER_LINEAR on 8-bit images: cv::resize -> resizeGeneric_ / HResizeLinear / VResizeLinear, fixed point
# ---------------------------------------------------------------------------------------------------------------------
def _cv_round_short(x: np.float32, half_up: bool) -> int:
    """``saturate_cast<short>(float)``: cvRound (to nearest, ties to even), then saturation."""
    v = math.floor(float(x) + 0.5) if half_up else int(round(float(x)))      # Python's round() is half-to-even
    return max(-32768, min(32767, v))


def _cv_axis(n_in: int, n_out: int, vertical: bool, variant: Optional[str]):
    """Per output coordinate (i0, i1, c0, c1)."""
    h_rule = (not vertical) or variant == "linear_h_rule_vertical"
    half_up = variant == "linear_round_half_up"
    inv_scale = float(n_out) / float(n_in)
    scale = 1.0 / inv_scale
    out = []
    for d in range(n_out):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(math.floor(float(f)))
        f = np.float32(f - np.float32(s))
        if h_rule:
            if s < 0:
                f, s = np.float32(0.0), 0
            if s >= n_in - 1:
                f, s = np.float32(0.0), n_in - 1
            i0, i1 = s, min(s + 1, n_in - 1)
        else:
            i0, i1 = min(max(s, 0), n_in - 1), min(max(s + 1, 0), n_in - 1)
        c0 = _cv_round_short(np.float32(np.float32(1.0) - f) * np.float32(2048.0), half_up)
        c1 = _cv_round_short(f * np.float32(2048.0), half_up)
        out.append((i0, i1, c0, c1))
    return out


def cv_linear_u8(imgs: np.ndarray, out_h: int, out_w: int, variant: Optional[str] = None) -> np.ndarray:
    """``cv2.resize(img, (out_w, out_h), interpolation=cv2.INTER_LINEAR)`` for every image of [n, h, w, 3] u8, pixel by pixel."""
    assert variant in (None, "linear_h_rule_vertical", "linear_round_half_up"), variant
    n, h, w, ch = imgs.shape
    xs = _cv_axis(w, out_w, False, variant)
    ys = _cv_axis(h, out_h, True, variant)
    src = imgs.tolist()
    out = np.empty((n, out_h, out_w, ch), dtype=np.uint8)
    for i in range(n):
        for dy, (y0, y1, b0, b1) in enumerate(ys):
            r0, r1 = src[i][y0], src[i][y1]
            for dx, (x0, x1, a0, a1) in enumerate(xs):
                for c in range(ch):
                    h0 = r0[x0][c] * a0 + r0[x1][c] * a1
                    h1 = r1[x0][c] * a0 + r1[x1][c] * a1
                    v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2
                    out[i, dy, dx, c] = 0 if v < 0 else (255 if v > 255 else v)
    return out


def exact_bilinear(imgs: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """Two-tap bilinear interpolation at ``(d + 0.5) * in / out - 0.5`` with replicated borders, in float64."""
    def axis(n_in, n_out):
        f = (np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5
        s = np.floor(f)
        return np.clip(s, 0, n_in - 1).astype(np.int64), np.clip(s + 1, 0, n_in - 1).astype(np.int64), f - s

    a = imgs.astype(np.float64)
    x0, x1, fx = axis(a.shape[2], out_w)
    y0, y1, fy = axis(a.shape[1], out_h)
    hor = a[:, :, x0] * (1.0 - fx)[None, None, :, None] + a[:, :, x1] * fx[None, None, :, None]
    return hor[:, y0] * (1.0 - fy)[None, :, None, None] + hor[:, y1] * fy[None, :, None, None]


# ---------------------------------------------------------------------------------------------------------------------
# stem, pools
# ---------------------------------------------------------------------------------------------------------------------
def stem_interior(bytes_: torch.Tensor) -> torch.Tensor:
    """[N, PH, PW, 3] u8 -> f32 ``u8 - PIXEL_MEAN`` (the values the kernels read)."""
    return bytes_.to(torch.float32) - torch.from_numpy(MEAN32)


def stem_input(bytes_: torch.Tensor) -> torch.Tensor:
    """The stem's input tensor [N, PH + 6, PW + 8, 4] f32: zero border (3 rows / columns in front, 3 / 5 behind), zero fourth channel."""
    n, ph, pw, _ = bytes_.shape
    x = torch.zeros((n, ph + 6, pw + 8, 4), dtype=torch.float32)
    x[:, 3:3 + ph, 3:3 + pw, :3] = stem_interior(bytes_)
    return x


def stem_reference(ops: Dict[str, torch.Tensor], variant: Optional[str] = None) -> torch.Tensor:
    """float64 ``relu(conv2d(x, w, stride 2, pad 3) * scale + bias)`` of the unbordered interior, NHWC [N, PH / 2, PW / 2, 64]."""
    assert variant in (None, "conv_pad2", "conv_phase"), variant
    x = stem_interior(ops["bytes"]).double().permute(0, 3, 1, 2)
    lo = {None: 3, "conv_pad2": 2, "conv_phase": 4}[variant]        # taps start at 2 o - lo; the far side keeps the output size
    y = F.conv2d(F.pad(x, (lo, 6 - lo, lo, 6 - lo)), ops["wt"].double(), stride=2)
    y = y * ops["scale"].double().view(1, -1, 1, 1) + ops["bias"].double().view(1, -1, 1, 1)
    return F.relu(y).permute(0, 2, 3, 1).contiguous()


def pool_reference(x: torch.Tensor, variant: Optional[str] = None) -> torch.Tensor:
    """``max_pool2d(3, 2, 1)`` of NHWC [N, H, W, C], in the dtype given (a maximum is exact in any)."""
    assert variant in (None, "pool_window_2o"), variant
    t = x.permute(0, 3, 1, 2)
    if variant is None:
        y = F.max_pool2d(t, 3, 2, 1)
    else:                                                   # windows 2 o .. 2 o + 2 instead of 2 o - 1 .. 2 o + 1
        ho, wo = S.pooled_extent(t.shape[2]), S.pooled_extent(t.shape[3])
        t = F.pad(t, (0, 2 * wo + 1 - t.shape[3], 0, 2 * ho + 1 - t.shape[2]), value=float("-inf"))
        y = F.max_pool2d(t, 3, 2, 0)
    return y.permute(0, 2, 3, 1).contiguous()


def p32_planes(y: torch.Tensor, s: float, groups: int, single: bool):
    """P32 of an f32 tensor [N, H, W, C] under the scale ``s`` (an exact power of two): (planes [pixels, C / 32, 2, 32] fp16, meta
    [groups, 2] = {max |y|, s}).  ``y * s`` is exact; ``h = half(y s)`` and ``l = half(y s - h)`` round to nearest even."""
    assert y.dtype == torch.float32 and math.frexp(s)[0] == 0.5
    c = y.shape[-1]
    ys = (y * s).reshape(-1, c // 32, 32)
    h = ys.to(torch.float16)
    l = torch.zeros_like(h) if single else (ys - h.to(torch.float32)).to(torch.float16)
    meta = torch.stack([y.reshape(groups, -1).abs().amax(dim=1), torch.full((groups,), s)], dim=1)
    return torch.stack([h, l], dim=2).contiguous(), meta
