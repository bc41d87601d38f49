"""Cases of the image front end (``csrc/preproc_stem.hip``) for ``test_gpu_front_end_edges.py``, and the rules that say which
kernel a case reaches.  Needs no GPU: ``test_cpu_front_end_ref.py`` checks the rules against the source and the references
against known answers.

The entries ``demia_resize_h_u8`` and ``demia_resize_v_norm`` each choose between two kernels at launch time:

  * horizontal: ``resize_h_row_kernel`` while a source row and its output row fit a 60 KiB LDS window, else the plain
    ``resize_h_kernel``; no launch at all when the width does not change (``tmp`` is then the source itself);
  * vertical: ``resize_v_norm4_kernel`` when ``newW % 4 == 0``, ``tmp`` is 4-byte aligned and ``DEMIA_RESIZE_PLAIN`` is not in
    the environment, else ``resize_v_norm_kernel``.

Both rules are restated here (``h_kernel``, ``v_kernel``); the horizontal one is compared with the expression in the source.
"""
from __future__ import annotations

import re
from pathlib import Path
from typing import List, NamedTuple, Tuple

import numpy as np
import torch

SOURCE = Path(__file__).resolve().parent.parent / "deepemia_amd" / "csrc" / "preproc_stem.hip"

BAR = 2e-5               # max-normalised error against f64: the bar of test_gpu_parity_nn.py and conv_p32_cases.BAR for f32 / P32 convolutions
TELL = 100.0             # a wrong conv / pool reference must be further than TELL * BAR from the right one

LDS_WINDOW = 60 * 1024


def row_kernel_lds_bytes(w: int, new_w: int) -> int:
    """Dynamic LDS of ``resize_h_row_kernel``: the source row behind up to 15 bytes of misalignment, rounded to 16, and the output row."""
    return ((w * 3 + 32 + 15) & ~15) + new_w * 3 + 8


def h_kernel(w: int, new_w: int) -> str:
    if w == new_w:
        return "none"
    return "row" if row_kernel_lds_bytes(w, new_w) <= LDS_WINDOW else "plain"


def v_kernel(new_w: int, tmp_offset: int = 0, plain_env: bool = False) -> str:
    return "norm4" if (new_w % 4 == 0 and tmp_offset % 4 == 0 and not plain_env) else "norm"


def parse_row_rule() -> Tuple[str, int]:
    """(the LDS size expression, the window in bytes) as ``demia_resize_h_u8`` states them, blanks removed."""
    text = SOURCE.read_text()
    body = text[text.index('extern "C" int demia_resize_h_u8'):]
    body = body[:body.index("\n}\n")]
    size = re.search(r"const long smem = (.+?);", body).group(1)
    window = re.search(r"if \(smem <= (\d+) \* (\d+)", body)
    return size.replace(" ", ""), int(window.group(1)) * int(window.group(2))


def parse_v_rule() -> str:
    text = SOURCE.read_text()
    body = text[text.index('extern "C" int demia_resize_v_norm'):]
    return re.search(r"\n    if \(([^\n]+)\) \{\n\s+hipLaunchKernelGGL\(resize_v_norm4_kernel", body).group(1).replace(" ", "")


# ---------------------------------------------------------------------------------------------------------------------
# 1. Pillow-exact resize
# ---------------------------------------------------------------------------------------------------------------------
class ResizeCase(NamedTuple):
    name: str
    n: int
    h: int
    w: int
    new_h: int
    new_w: int
    src_off: int = 0           # byte offset of the source inside a larger buffer of random bytes (on top of a 16-byte aligned base)
    content: str = "random"    # random | zeros | ones | checker
    gen_w: int = 0             # width at which random content is drawn (then cut to w): two cases share their left columns

    @property
    def ph(self) -> int:
        return (self.new_h + 31) // 32 * 32

    @property
    def pw(self) -> int:
        return (self.new_w + 31) // 32 * 32

    @property
    def hk(self) -> str:
        return h_kernel(self.w, self.new_w)

    @property
    def vk(self) -> str:
        return v_kernel(self.new_w, self.src_off if self.w == self.new_w else 0)


def _lds_pair(new_w: int) -> Tuple[int, int]:
    """The widest source row that still takes the row kernel for ``new_w`` output pixels, and the next one."""
    w = new_w + 1
    while h_kernel(w + 1, new_w) == "row":
        w += 1
    return w, w + 1


LDS_UNDER, LDS_OVER = _lds_pair(1333)          # 19130 and 19131: 14.35 source pixels per output pixel, 31 taps

RESIZE_CASES: List[ResizeCase] = [
    # both horizontal kernels on the same content, either side of the LDS rule, and two realistic widths
    ResizeCase("lds-under", 1, 3, LDS_UNDER, 3, 1333, gen_w=LDS_OVER),
    ResizeCase("lds-over", 1, 3, LDS_OVER, 3, 1333, gen_w=LDS_OVER),
    ResizeCase("wide-20000", 2, 2, 20000, 2, 1333, src_off=5),
    ResizeCase("moderate-4100", 2, 3, 4100, 3, 800, src_off=1),
    # alignment: W * 3 = 111 (15 mod 16), H * W * 3 = 555 (11 mod 16): rows and images start at every residue; the last row's final
    # 16-byte load crosses the end of the source; newW * 3 on every residue mod 4
    ResizeCase("align-off0", 3, 5, 37, 4, 21, src_off=0),
    ResizeCase("align-off1", 3, 5, 37, 3, 22, src_off=1),
    ResizeCase("align-off5", 3, 5, 37, 5, 23, src_off=5),
    ResizeCase("align-off15", 3, 5, 37, 2, 20, src_off=15),
    ResizeCase("align-up-off15", 2, 3, 7, 8, 19, src_off=15),
    # scale factors
    ResizeCase("upscale", 2, 5, 7, 13, 18),
    ResizeCase("down-13-taps", 1, 100, 101, 17, 18),          # 5.88 and 5.61 source pixels per output pixel: 13 taps
    ResizeCase("down-200-13", 2, 200, 200, 13, 13, src_off=1),  # 15.4: 33 taps
    ResizeCase("in1-out1", 1, 1, 1, 1, 1),
    ResizeCase("in1-out5", 3, 1, 1, 5, 5, src_off=1),
    ResizeCase("in2x3-out1", 3, 2, 3, 1, 1, src_off=5),
    ResizeCase("same-w-1333", 1, 301, 1333, 300, 1333, src_off=1),     # need_h false: tmp is the (misaligned) source, plain vertical kernel
    ResizeCase("same-w-36", 2, 41, 36, 30, 36),                        # the same, aligned: the four-pixel vertical kernel
    ResizeCase("same-h-300", 1, 300, 1334, 300, 1333),                   # one tap of 1 << 22 per output row
    ResizeCase("same-w-300", 2, 1334, 300, 1333, 300, src_off=15),      # its transpose: need_h false again
    ResizeCase("identity-both", 3, 9, 12, 9, 12, src_off=5),
    # content: clip8 and the rounding constant
    ResizeCase("zeros-down", 1, 23, 37, 9, 14, content="zeros"),
    ResizeCase("ones-down", 2, 23, 37, 9, 14, content="ones"),
    ResizeCase("checker-down", 1, 23, 37, 9, 14, content="checker"),
    ResizeCase("zeros-up", 1, 6, 5, 15, 13, content="zeros"),
    ResizeCase("ones-up", 1, 6, 5, 15, 13, content="ones"),
    ResizeCase("checker-up", 2, 6, 5, 15, 13, content="checker"),
    ResizeCase("checker-wide", 1, 2, LDS_OVER, 2, 1333, content="checker"),
]

# both vertical kernels on the same input: newW % 4 == 0 with and without DEMIA_RESIZE_PLAIN=1, with tmp moved on by one byte,
# and newW on the other residues
V_PAIR = ResizeCase("v-pair", 2, 23, 50, 17, 36, src_off=1)
V_MOD = [ResizeCase(f"v-mod{r}", 2, 23, 50, 17, 36 + r) for r in (1, 2, 3)]

# sizes replayed on the CPU only (one axis each): tables of 1 and 5127 taps among them
REPLAY_SIZES = [(1, 5), (2, 1), (3, 1), (20500, 8), (20000, 1333), (4100, 800), (801, 800), (7, 7), (200, 13), (5, 13)]


def resize_images(case: ResizeCase) -> np.ndarray:
    """[n, h, w, 3] u8.  Images of a batch differ."""
    shape = (case.n, case.h, case.w, 3)
    if case.content == "zeros":
        return np.zeros(shape, dtype=np.uint8)
    if case.content == "ones":
        return np.full(shape, 255, dtype=np.uint8)
    if case.content == "checker":
        y, x, c = np.meshgrid(np.arange(case.h), np.arange(case.w), np.arange(3), indexing="ij")
        one = (((y + x + c) & 1) * 255).astype(np.uint8)
        return np.stack([one if i % 2 == 0 else 255 - one for i in range(case.n)])
    gen_w = case.gen_w or case.w
    rng = np.random.default_rng(1000 + case.h * 7 + gen_w)
    return np.ascontiguousarray(rng.integers(0, 256, size=(case.n, case.h, gen_w, 3), dtype=np.uint8)[:, :, :case.w])


# ---------------------------------------------------------------------------------------------------------------------
# 2. OpenCV INTER_LINEAR, 8 bit
# ---------------------------------------------------------------------------------------------------------------------
class LinearCase(NamedTuple):
    name: str
    n: int
    h: int
    w: int
    oh: int
    ow: int


LINEAR_CASES: List[LinearCase] = [
    LinearCase("x2", 1, 6, 9, 12, 18),
    LinearCase("x1.5", 2, 8, 10, 12, 15),
    LinearCase("x0.75", 1, 12, 16, 9, 12),
    LinearCase("x0.5", 1, 10, 14, 5, 7),
    LinearCase("odd-37-55-101-67", 1, 37, 101, 55, 67),
    LinearCase("odd-101-67-37-55", 1, 101, 37, 67, 55),
    LinearCase("odd-5-9", 3, 5, 5, 9, 9),
    LinearCase("src1", 1, 1, 1, 4, 3),
    LinearCase("src1-row", 2, 1, 7, 3, 7),
    LinearCase("src2", 1, 2, 2, 5, 7),
    LinearCase("out1", 1, 9, 6, 1, 1),
    LinearCase("out1-h", 2, 4, 7, 1, 5),
    LinearCase("edge-rules", 3, 6, 6, 9, 9),        # the two edge rules give different bytes for the extent pair 6 -> 9
]
EDGE_RULE_CASE = "edge-rules"
LINEAR_MAX_EXTENT = 128                             # no case has a coordinate beyond this (enters the derived bound)


def linear_images(case: LinearCase) -> np.ndarray:
    rng = np.random.default_rng(2000 + case.h * 131 + case.w * 7 + case.oh)
    return rng.integers(0, 256, size=(case.n, case.h, case.w, 3), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------------
# 3. stem, pools, subsample
# ---------------------------------------------------------------------------------------------------------------------
PIXEL_MEAN = (103.530, 116.280, 123.675)            # compared with engine.PIXEL_MEAN by the CPU test


class StemCase(NamedTuple):
    ph: int
    pw: int
    n: int

    @property
    def name(self) -> str:
        return f"{self.ph}x{self.pw}-n{self.n}"


# conv outputs 16 x 16 (exactly one tile; the pooled 8 x 8 is 7 + 1), 16 x 32, 32 x 16, 32 x 48, 48 x 80; the fused kernel's
# own 16 x 16 conv tile starts one position early, so for it 16 conv rows are already two tiles
STEM_SIZES = [(32, 32), (32, 64), (64, 32), (64, 96), (96, 160)]
STEM_CASES = [StemCase(ph, pw, n) for ph, pw in STEM_SIZES for n in (1, 3)]
ZERO_CHANNEL = 7


def stem_operands(case: StemCase):
    """dict: bytes [N, PH, PW, 3] u8, wt [64, 3, 7, 7], scale [64], bias [64] (f32, CPU).  Magnitudes per channel over three
    decades, channel ZERO_CHANNEL all zero, every fifth scale negative, biases that push a third of the channels below zero."""
    g = torch.Generator().manual_seed(3000 + case.ph * 3 + case.pw)
    bytes_ = torch.randint(0, 256, (3, case.ph, case.pw, 3), generator=g, dtype=torch.uint8)[:case.n].contiguous()
    mag = 10.0 ** (-3.0 + 3.0 * torch.rand((64,), generator=g))
    wt = torch.randn((64, 3, 7, 7), generator=g) * (0.02 * mag).view(64, 1, 1, 1)
    wt[ZERO_CHANNEL] = 0
    scale = torch.rand((64,), generator=g) + 0.5
    scale[::5] *= -1
    spread = 0.02 * mag * 75.0 * 147 ** 0.5 * scale.abs()           # roughly the standard deviation of the scaled conv output
    bias = torch.randn((64,), generator=g) * 0.3 * spread
    bias[1::3] -= spread[1::3]
    bias[ZERO_CHANNEL] = 0.25
    return dict(bytes=bytes_, wt=wt, scale=scale, bias=bias)


def stem_bound(ops) -> float:
    """The a-priori bound of the stem output (``engine.py::_pack``): the P32 scale of the pooled tensor comes from it."""
    wt, scale, bias = ops["wt"], ops["scale"], ops["bias"]
    return float(((255.0 - min(PIXEL_MEAN)) * scale.abs() * wt.abs().flatten(1).sum(1) + bias.abs()).max())


class PoolCase(NamedTuple):
    n: int
    h: int
    w: int
    c: int

    @property
    def name(self) -> str:
        return f"n{self.n}-{self.h}x{self.w}-c{self.c}"


POOL_P32_CASES = [PoolCase(3, 7, 10, 64), PoolCase(2, 8, 5, 256), PoolCase(1, 1, 1, 64), PoolCase(3, 16, 16, 64), PoolCase(2, 25, 42, 256)]
POOL_CASES = [PoolCase(2, 25, 42, 256), PoolCase(1, 1, 1, 256), PoolCase(3, 8, 6, 64), PoolCase(1, 2, 1, 4), PoolCase(2, 7, 16, 64)]


def pool_input(case: PoolCase, amplitude: float = 3.0) -> torch.Tensor:
    """[N, H, W, C] f32 with both signs; image i is 10^i times larger than image 0.  The upper half of the last image's channels
    is negative throughout and large, so that the largest |pooled value| of the tensor (and of that image) is a NEGATIVE one:
    a maximum taken without the absolute value gives another ``meta``."""
    g = torch.Generator().manual_seed(4000 + case.h * 50 + case.w + case.c)
    x = torch.randn((case.n, case.h, case.w, case.c), generator=g) * amplitude
    x[-1, :, :, case.c // 2:] = -(40.0 * amplitude + x[-1, :, :, case.c // 2:].abs())
    return x * (10.0 ** torch.arange(case.n, dtype=torch.float32)).view(-1, 1, 1, 1)


def pooled_extent(n: int) -> int:
    return (n + 2 - 3) // 2 + 1


VARIANTS = ("conv_pad2", "conv_phase", "pool_window_2o", "linear_h_rule_vertical", "linear_round_half_up", "pillow_no_rounding")
