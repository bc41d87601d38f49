"""The named boxes the ROI pooler is tested on (``test_cpu_roi_align_ref.py``, ``test_gpu_roi_align_edges.py``): one small
pyramid of a 512 x 160 px image (height x width), two images, and a table of boxes in which every entry names the branch
of ``csrc/roialign.hip`` it exists for.  ``expect`` is what the reference's own diagnostics must say about the box AT
``expect["P"]`` (the CPU test checks it, so that a case cannot quietly stop reaching its branch); every box is pooled at
every ``P`` of the tests all the same.

Every box is finite and at most a few thousand pixels on a side: non-finite and negative-area boxes never reach the
pooler (the proposal and detection kernels drop them).
"""
from collections import namedtuple

import numpy as np

IMG_H, IMG_W = 512, 160
SIZES = ((128, 40), (64, 20), (32, 10), (16, 5))        # (H, W) of p2 .. p5
C = 256
N_IMAGES = 2
POOL_SIZES = (1, 2, 7, 14, 15)

# Largest |oracle - reference| / amax(level features) over this table, both images, 256 channels and POOL_SIZES, where the
# oracle is oracle.maskrcnn_ref.roi_pool (torch f32, another summation order) and the reference tests/roi_align_ref.py
# (f64 sums).  Measured by test_cpu_roi_align_ref.py: 1.319e-7, at bulk_22 with P = 15 in image 0 (that test prints the
# figure and fails when it leaves this record).  The GPU tolerances are derived from it.
ORACLE_VS_REF = 1.32e-7

Case = namedtuple("Case", "name box expect why")


def _h(s: str) -> float:
    return float.fromhex(s)


def features(seed: int = 20):
    """Four arrays [N_IMAGES, H, W, C] float32: randn * 3, five channels three orders of magnitude smaller."""
    rng = np.random.default_rng(seed)
    out = []
    for (h, w) in SIZES:
        x = (rng.standard_normal((N_IMAGES, h, w, C)) * 3.0).astype(np.float32)
        x[..., :5] *= np.float32(1e-3)
        out.append(x)
    return out


def _level_cases():
    cases = []
    # sqrt(area) exactly on a level boundary, in non-square shapes, and one side a pixel shorter / longer
    for root, (w, h), (x0, y0), lv in ((112, (56, 224), (40, 100), 1), (224, (112, 448), (20, 30), 2), (448, (224, 896), (-30, -100), 3)):
        cases.append(Case(f"level_sqrt_area_{root}_exact", (x0, y0, x0 + w, y0 + h), dict(P=7, level=lv),
                          f"{w} x {h}: sqrt(area) = {root} exactly, the first box of p{lv + 2}"))
        cases.append(Case(f"level_sqrt_area_{root}_minus_1px", (x0, y0, x0 + w, y0 + h - 1), dict(P=7, level=lv - 1),
                          f"{w} x {h - 1}: just under {root}, the last of p{lv + 1}"))
        cases.append(Case(f"level_sqrt_area_{root}_plus_1px", (x0, y0, x0 + w + 1, y0 + h), dict(P=7, level=lv),
                          f"{w + 1} x {h}: just over {root}"))
    cases.append(Case("level_2x2_clamps_to_p2", (70, 300, 72, 302), dict(P=7, level=0, gy=1, gx=1), "log2 gives level 0: clamped up"))
    cases.append(Case("level_1500x1400_clamps_to_p5", (-600, -500, 900, 900), dict(P=7, level=3), "log2 gives level 6: clamped down"))
    cases.append(Case("zero_width", (50, 30, 50, 90), dict(P=7, level=0, gx=0, zero=True),
                      "a detection box clipped to nothing: gw = 0, count = max(0, 1), output 0 at p2"))
    cases.append(Case("zero_height", (30, 50, 90, 50), dict(P=7, level=0, gy=0, zero=True), "gh = 0"))
    return cases


def _path_cases():
    return [
        Case("tables_gh7_gw2", (60, 4, 100, 200), dict(P=7, level=0, gy=7, gx=2), "the largest grid of the separable path"),
        Case("fallback_gh8_gw2", (60, 4, 100, 204), dict(P=7, level=0, gy=8, gx=2), "four pixels taller: the per-sample path"),
        Case("tables_gw7_gh2", (4, 60, 200, 100), dict(P=7, level=0, gy=2, gx=7), "the transpose (its right part hangs over the image)"),
        Case("fallback_gw8_gh2", (4, 60, 204, 100), dict(P=7, level=0, gy=2, gx=8), "the transpose"),
        # (at P = 7 a box with 7 x 7 samples per bin is 196 px square and goes to p3, where it has 4 x 4: P = 2 reaches it)
        Case("tables_gh7_gw7_at_P2", (60, 100, 116, 156), dict(P=2, level=0, gy=7, gx=7), "7 x 7 samples per bin, still tables"),
        Case("fallback_gh8_gw8_at_P2", (60, 100, 120, 160), dict(P=2, level=0, gy=8, gx=8), "8 x 8: per-sample"),
        Case("fallback_P14_gh8", (70, 50, 90, 450), dict(P=14, level=0, gy=8, gx=1), "a mask box 400 px tall and 20 wide"),
        Case("fallback_gh15", (60, 4, 80, 400), dict(P=7, level=0, gy=15, gx=1), "15 samples down each bin"),
    ]


def _edge_cases():
    return [
        Case("sample_at_minus_1_y", (40, -4, 68, 24), dict(P=7, level=0, gy=1, has_y=-1.0, skipped_y=0),
             "rows at -1, 0 .. 5: -1 is not < -1, kept and clamped to row 0"),
        Case("sample_at_size_y", (40, 488, 68, 516), dict(P=7, level=0, gy=1, has_y=128.0, skipped_y=0),
             "rows at 122 .. 128: 128 is not > H, kept and clamped to row 127"),
        Case("sample_at_minus_1_x", (-4, 300, 24, 328), dict(P=7, level=0, gx=1, has_x=-1.0, skipped_x=0), "the same for columns"),
        Case("sample_at_size_x", (136, 300, 164, 328), dict(P=7, level=0, gx=1, has_x=40.0, skipped_x=0), "columns at 34 .. 40"),
        Case("sample_just_past_minus_1_y", (40, -4.25, 68, 23.75), dict(P=7, level=0, gy=1, skipped_y=1), "rows at -1.0625 ..: the first is dropped"),
        Case("sample_just_past_size_x", (136.25, 300, 164.25, 328), dict(P=7, level=0, gx=1, skipped_x=1), "columns .. 40.0625: the last is dropped"),
        Case("over_left_edge_by_a_third", (-20, 200, 40, 260), dict(P=7, level=0), "clamped and dropped columns on the left"),
        Case("over_right_edge_by_a_third", (120, 200, 180, 260), dict(P=7, level=0), "on the right"),
        Case("over_top_edge_by_a_third", (50, -20, 110, 40), dict(P=7, level=0), "rows at the top"),
        Case("over_bottom_edge_by_a_third", (50, 472, 110, 532), dict(P=7, level=0), "rows at the bottom"),
        Case("wholly_outside", (600, 600, 640, 640), dict(P=7, level=0, all_skipped=True, zero=True), "every sample dropped: zero output, no pixel read"),
        Case("empty_left_bin_live_right_bin", (-46, 100, 38, 150), dict(P=7, level=0, gx=3, touched_x={2: 0, 3: 2}),
             "columns: bins 0 .. 2 wholly left of -1, bin 3 has one sample at -0.5 -- an empty left bin beside a live right one in the "
             "column pair (2, 3); at P = 14 the pair is (6, 7)"),
        Case("empty_last_bins", (100, 400, 240, 440), dict(P=7, level=0, gx=5), "columns: the last bins wholly right of W"),
    ]


# Bins of 7 samples that touch NINE feature pixels (float32: the last sample's coordinate rounds up onto an integer while
# the first stays below one).  All at p2 (scale 1/4); the other axis is short enough to keep the box there.  Found by a
# seeded search over box edges one to eight float32 steps under a multiple of 4 with the reference's own geometry
# (tests/roi_align_ref.axis_samples); the coordinates are the literals it printed, the first five those of the report of
# the defect.  Every hit has a power of two strictly inside the bin's pixel range (where the float32 step doubles); on this
# 128 x 40 map the search found rows in bins 0 .. 4 of 7 and 0 .. 8 of 14 -- "last" below is the last bin it found -- and
# columns in the first bins only (the later ones lie beyond the map's 40 columns).
_NINE = (
    # name, axis, P, c1, c2, bin
    ("nine_rows_P7_bin0", "y", 7, "0x1.bffffe0000000p+5", "0x1.f800000000000p+7", 0),    # 55.999996 .. 252
    ("nine_rows_P7_bin3", "y", 7, "0x1.bffff80000000p+4", "0x1.c000000000000p+7", 3),    # 27.999992 .. 224
    ("nine_rows_P7_bin1", "y", 7, "0x1.6ffffe0000000p+6", "0x1.2000000000000p+8", 1),    # 91.999992 .. 288
    ("nine_rows_P14_bin6", "y", 14, "0x1.1ffffc0000000p+6", "0x1.cffffe0000000p+8", 6),    # 71.999985 .. 463.99997
    ("nine_rows_P14_bin1", "y", 14, "0x1.a7fffe0000000p+7", "0x1.2e00000000000p+9", 1),    # 211.99998 .. 604
    ("nine_rows_P7_bin0_at_top", "y", 7, "0x1.fffffe0000000p+1", "0x1.9000000000000p+7", 0),    # 3.9999998 .. 200
    ("nine_rows_P7_bin2", "y", 7, "0x1.1ffffe0000000p+6", "0x1.0c00000000000p+8", 2),    # 71.999992 .. 268
    ("nine_rows_P7_bin4_last", "y", 7, "0x1.7ffff60000000p+3", "0x1.a000000000000p+7", 4),    # 11.999995 .. 208
    ("nine_rows_P14_bin0", "y", 14, "0x1.fffff80000000p+1", "0x1.8c00000000000p+8", 0),    # 3.999999 .. 396
    ("nine_rows_P14_bin4", "y", 14, "0x1.fffffc0000000p+6", "0x1.0400000000000p+9", 4),    # 127.99998 .. 520
    ("nine_rows_P14_bin8_last", "y", 14, "0x1.3ffff60000000p+4", "0x1.9c00000000000p+8", 8),    # 19.99999 .. 412
    ("nine_cols_P7_bin0", "x", 7, "0x1.fffffe0000000p+5", "0x1.0400000000000p+8", 0),    # 63.999996 .. 260
    ("nine_cols_P7_bin1", "x", 7, "0x1.6ffffe0000000p+6", "0x1.2000000000000p+8", 1),    # 91.999992 .. 288
    ("nine_cols_P7_bin2", "x", 7, "0x1.bffffc0000000p+5", "0x1.f800000000000p+7", 2),    # 55.999992 .. 252
    ("nine_cols_P7_bin3", "x", 7, "0x1.7ffffa0000000p+4", "0x1.b800000000000p+7", 3),    # 23.999994 .. 220
    ("nine_cols_P14_bin0", "x", 14, "0x1.7ffffe0000000p+5", "0x1.b800000000000p+8", 0),    # 47.999996 .. 440
    ("nine_cols_P14_bin2", "x", 14, "0x1.0ffffe0000000p+6", "0x1.cc00000000000p+8", 2),    # 67.999992 .. 460
)


def _nine_cases():
    cases = []
    for name, axis, P, c1, c2, b in _NINE:
        c1, c2 = _h(c1), _h(c2)
        short = (20.0, 60.0) if P == 7 else (20.0, 44.0)                 # 40 or 24 px: sqrt(area) < 112
        box = (short[0], c1, short[1], c2) if axis == "y" else (c1, short[0] + 200.0, c2, short[1] + 200.0)
        expect = dict(P=P, level=0, nine=(axis, b))
        expect["gy" if axis == "y" else "gx"] = 7
        cases.append(Case(name, box, expect, f"bin {b} of the {'rows' if axis == 'y' else 'columns'} touches 9 pixels with 7 samples"))
    return cases


def _bulk_cases(n: int = 60, seed: int = 5):
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        size = float(np.exp(rng.uniform(np.log(6.0), np.log(400.0))))
        asp = float(np.exp(rng.uniform(np.log(0.1), np.log(10.0))))
        cx, cy = float(rng.uniform(-10.0, IMG_W - 10.0)), float(rng.uniform(-10.0, IMG_H - 10.0))
        w, h = size * asp ** 0.5, size / asp ** 0.5
        cases.append(Case(f"bulk_{i:02d}", (cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2), dict(P=7), "seeded random box"))
    return cases


CASES = _level_cases() + _path_cases() + _edge_cases() + _nine_cases() + _bulk_cases()
NAMES = [c.name for c in CASES]
BOXES = np.array([c.box for c in CASES], dtype=np.float32)          # [R, 4] (x1, y1, x2, y2)
R = len(CASES)
assert len(set(NAMES)) == R
