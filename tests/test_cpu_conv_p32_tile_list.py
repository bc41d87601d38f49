"""The parts of the P32 tile sweep (``test_gpu_conv_p32_tiles.py``) that need no GPU.

  * the tile ids the GPU module sweeps are the ones ``conv_p32.hip`` instantiates for the product: ``kTiles`` and the two
    dispatch switches are parsed from the source, so a tile added later cannot go untested silently;
  * the per-tile row counts reach what they are chosen for: one partial tile, whole tiles exactly, a ragged remainder that
    is no multiple of 32, and a workgroup count on every residue mod 8 (``xcd_remap``), values below 8 included;
  * the float64 reference can tell: for every case it lies further than 100x the bar from each deliberately wrong variant
    (no residual, nearest-2x residual with floor instead of ceil, last tap / last 32-channel group dropped, padding off by
    one, scale and bias rolled by one channel) and from itself shifted by one row.
"""
import pytest
import torch

import conv_p32_cases as S


def test_swept_tiles_are_the_product_tiles():
    ktiles = S.parse_ktiles()
    plain, guarded = S.parse_dispatch()
    assert ktiles == S.PLANE_TILES, (ktiles, S.PLANE_TILES)
    assert plain == S.PLANE_TILES, (plain, S.PLANE_TILES)            # every kTiles entry has its case in the switch, with that shape
    assert guarded == S.GUARDED_TILES, (guarded, S.GUARDED_TILES)
    swept = {t.name for t, _ in S.SWEEP}
    assert swept == {str(i) for i in ktiles} | {f"{i}G" for i in guarded}
    # every swept tile has cases that are launched, not only refused ones
    for t in S.TILES:
        assert sum(not S.refused(t, c) for tt, c in S.SWEEP if tt == t) >= 8, t.name


def test_the_guarded_tile_reachable_by_hint_only_is_still_that_one():
    """Tile 10G is in the guarded switch but neither ``choose_tile`` (it is not in kTiles) nor the fall-back of a hint that
    has no guarded instantiation (7 or 11) ever selects it."""
    assert S.GUARDED_BY_HINT_ONLY == set(S.GUARDED_TILES) - set(S.parse_ktiles())
    text = S.SOURCE.read_text()
    assert "tile = n128 ? 7 : 11;" in text


@pytest.mark.parametrize("tile", S.TILES, ids=lambda t: t.name)
def test_row_counts_reach_every_residue_and_edge(tile):
    mine = [(c, S.rows_for(tile, c)) for t, c in S.SWEEP if t == tile and not S.refused(t, c)]
    counts = [S.nwg(tile, c, n) for c, n in mine]
    assert {w % 8 for w in counts} == set(range(8)), sorted(counts)
    assert any(w < 8 for w in counts) and max(counts) >= 520, sorted(counts)
    ms = [n * c.ho * c.wo for c, n in mine]
    assert any(m < tile.bm for m in ms)
    assert any(m % tile.bm == 0 for m in ms)
    assert any(m % tile.bm % 32 != 0 for m in ms)


def test_channel_counts_of_the_sweep():
    def couts(name):
        return {c.cout for t, c in S.SWEEP if t.name == name and not S.refused(t, c)}
    for name in ("1", "2", "4", "12", "13"):
        assert couts(name) == {256, 512}
    for name in ("6", "7"):
        assert couts(name) == {128, 256, 384, 512}
    for name in ("9", "11"):
        assert couts(name) == {64, 128, 192, 256, 384, 512}
    for name in ("9G", "10G", "11G"):
        assert {15, 80, 96} <= couts(name)
    assert {80, 96} <= couts("7G")
    assert {(c.cout, c.out_f32, c.ld) for c in S.CASES if c.guarded} >= {(15, True, 16), (80, True, 80), (96, False, 96)}


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_the_reference_can_tell(case):
    n = min(S.n_common(case), 2048 if case.h * case.w == 1 else 6)
    ops = S.operands(case, n)
    ref = S.reference(case, ops)
    amax = float(ref.abs().max())
    assert amax > 0
    for v in S.variants_of(case):
        d = float((S.reference(case, ops, v) - ref).abs().max()) / amax
        assert d > S.TELL * S.BAR, (v, d)
    # and an output that is right except for ONE element off by 3x the bar does not pass
    wrong = ref.clone()
    wrong[-1, -1] += 3 * S.BAR * amax
    assert S.normalised_error(wrong, ref) > S.BAR


def test_operands_span_the_stated_ranges():
    exps = {c.amp_exp for c in S.CASES}
    assert min(exps) == -3 and max(exps) == 3
    assert {c.relu for c in S.CASES} == {True, False}
    for c in S.CASES:
        ops = S.operands(c, 4)
        assert 0.5 <= float(ops["scale"].min()) and float(ops["scale"].max()) <= 1.5
        assert ops["bias"].unique().numel() == c.cout


# What ``tile_hint = 0`` resolves to for the kernel-level tests that never pass a hint (restated cost model, CPU only):
# CONV_CASES of test_gpu_parity_nn.py, then the cases of test_conv_p32_scale_groups_equal_the_images_alone.
CONV_CASES_AUTO = ["11", "11", "11", "11", "11", "11G", "11", "11", "4", "11", "1"]
GROUP_CASES_AUTO = ["11", "11", "11G", "11"]


def test_what_the_older_kernel_tests_cover():
    conv = [(64, 64, 1, 1, 0, 50, 50, 2, True, 0), (64, 256, 1, 1, 0, 37, 41, 1, False, 1), (256, 128, 1, 2, 0, 50, 50, 2, True, 0),
            (64, 64, 3, 1, 1, 33, 29, 2, True, 0), (128, 128, 3, 1, 1, 25, 25, 3, True, 0), (256, 15, 1, 1, 0, 13, 13, 2, False, 0),
            (256, 256, 3, 1, 1, 14, 14, 5, True, 0), (512, 256, 1, 1, 0, 50, 50, 1, False, 2), (64, 256, 3, 1, 1, 300, 300, 1, True, 1),
            (128, 192, 3, 2, 1, 61, 47, 2, True, 0), (64, 256, 1, 1, 0, 512, 512, 1, True, 1)]
    got = []
    for cin, cout, k, stride, pad, h, w, n, _, res in conv:
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        got.append(S.resolve(0, n * ho * wo, cin, cout, k, res != 0, cout % 32 != 0))
    assert got == CONV_CASES_AUTO, got
    groups = [(3, 64, 64, 12, 12, 3, 1, 1, 1), (5, 32, 128, 16, 9, 1, 1, 0, 2), (2, 64, 96, 31, 17, 3, 2, 1, 0), (4, 128, 256, 13, 13, 3, 1, 1, 0)]
    got = []
    for n, cin, cout, h, w, k, stride, pad, res in groups:
        ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        got.append(S.resolve(0, n * ho * wo, cin, cout, k, res != 0, False))
    assert got == GROUP_CASES_AUTO, got


def test_tiles_the_model_selects_are_swept():
    """DESIGN.md section 4 quotes these histograms (R101-FPN, 800 x 800 inputs)."""
    swept = {t.name for t in S.TILES}
    quoted = {1: {"11": 106, "12": 7, "11G": 6, "7": 5, "2": 4},
              16: {"12": 53, "13": 27, "1": 18, "11": 8, "9": 6, "2": 6, "7": 4, "11G": 4, "9G": 2},
              48: {"1": 102, "9": 6, "7": 4, "6": 4, "2": 3, "9G": 3, "11G": 3, "4": 2, "11": 1}}
    for images in (1, 16, 48):
        hist = S.auto_tiles(images)
        assert set(hist) <= swept, hist
        assert "10G" not in hist
        assert hist == quoted[images], (images, hist)
