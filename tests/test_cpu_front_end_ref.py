"""The parts of the front-end tests (``test_gpu_front_end_edges.py``) that need no GPU.

  * the rules of ``front_end_cases.py`` that say which resize kernel a case reaches are the ones in ``preproc_stem.hip``, and the
    case list reaches both kernels of both passes, every alignment and every output phase it is chosen for;
  * a NumPy replay of Pillow's two integer passes from ``engine.pil_bilinear_tables`` equals the installed Pillow on every
    resize case and on single-axis sizes up to a 5127-tap table: the host tables are not the suspect;
  * the scalar restatement of OpenCV's 8-bit ``INTER_LINEAR`` gives known answers (identity, constants, a 2x upscale worked
    out by hand, the 2 x 2 box mean at factor 0.5), equals ``oracle/pipeline_ref.py::cv_resize_linear_u8`` and
    ``engine.cv_linear_tables`` on every case, and stays within the DERIVED bound ``front_end_ref.LINEAR_BOUND`` of exact
    float64 bilinear interpolation;
  * every reference can fail: each named mistake of ``front_end_cases.VARIANTS`` moves the result past the pass rule.

Largest distance of the restatement from exact bilinear over the cases: 0.7758 grey levels (derived bound 1.264).
"""
import re

import numpy as np
import pytest
import torch

import front_end_cases as S
import front_end_ref as R

ALL_RESIZE = S.RESIZE_CASES + [S.V_PAIR] + S.V_MOD


# ---------------------------------------------------------------------------------------------------------------------
# the rules and what the cases reach
# ---------------------------------------------------------------------------------------------------------------------
def test_the_row_rule_is_the_one_in_the_source():
    size, window = S.parse_row_rule()
    assert window == 60 * 1024 == S.LDS_WINDOW
    assert size == "(((long)W*3+32+15)&~15L)+(long)newW*3+8"
    for w, new_w in [(1, 1), (5, 3), (19130, 1333), (19131, 1333), (20000, 1333), (4100, 800)]:
        assert S.row_kernel_lds_bytes(w, new_w) == (((w * 3 + 32 + 15) & ~15) + new_w * 3 + 8)
    assert S.parse_v_rule() == '(newW&3)==0&&(reinterpret_cast<unsignedlonglong>(tmp)&3ull)==0&&!getenv("DEMIA_RESIZE_PLAIN")'
    # the kernel's own view of its LDS: the input part is the same rounded size, and the widest 16-byte store ends inside it
    text = S.SOURCE.read_text()
    assert "const int in_sz = (W * 3 + 32 + 15) & ~15;" in text
    assert "const int nbytes = W * 3 + mis;" in text


def test_the_cases_reach_both_kernels_of_both_passes():
    assert (S.LDS_UNDER, S.LDS_OVER) == (19130, 19131)
    by = {c.name: c for c in ALL_RESIZE}
    assert by["lds-under"].hk == "row" and by["lds-over"].hk == "plain"
    assert S.row_kernel_lds_bytes(S.LDS_UNDER, 1333) <= S.LDS_WINDOW < S.row_kernel_lds_bytes(S.LDS_OVER, 1333)
    assert by["wide-20000"].hk == "plain" and by["moderate-4100"].hk == "row" and by["checker-wide"].hk == "plain"
    assert {c.hk for c in ALL_RESIZE} == {"row", "plain", "none"}
    assert {c.vk for c in ALL_RESIZE} == {"norm4", "norm"}
    assert {c.n for c in ALL_RESIZE} == {1, 2, 3}
    # need_h false: tmp is the source, aligned (four-pixel kernel) and misaligned (plain kernel)
    assert (by["same-w-36"].hk, by["same-w-36"].vk) == ("none", "norm4")
    assert (by["same-w-300"].hk, by["same-w-300"].vk) == ("none", "norm")
    assert (by["same-w-1333"].hk, by["same-w-1333"].vk) == ("none", "norm")
    assert (by["same-h-300"].h, by["same-h-300"].w) == (by["same-w-300"].w, by["same-w-300"].h) == (300, 1334)
    assert by["identity-both"].hk == "none" and by["identity-both"].h == by["identity-both"].new_h
    assert S.V_PAIR.vk == "norm4" and S.v_kernel(S.V_PAIR.new_w, 1) == "norm" and S.v_kernel(S.V_PAIR.new_w, 0, True) == "norm"
    assert {c.new_w % 4 for c in S.V_MOD} == {1, 2, 3} and {c.vk for c in S.V_MOD} == {"norm"}


def test_the_alignment_cases_cover_every_residue():
    al = [c for c in S.RESIZE_CASES if c.name.startswith("align-off")]
    assert {c.src_off for c in al} == {0, 1, 5, 15}
    assert {c.new_w * 3 % 4 for c in al} == {0, 1, 2, 3}
    for c in al:
        assert c.hk == "row" and c.n == 3
        assert c.w * 3 % 16 and c.h * c.w * 3 % 16
        starts = {(c.src_off + r * c.w * 3) % 16 for r in range(c.n * c.h)}
        assert len(starts) >= 12, sorted(starts)
    # the last row's final 16-byte load from the aligned address below it would cross the end of the source (all but offset 15)
    assert [c.src_off for c in al if (c.src_off + c.n * c.h * c.w * 3) % 16 != 0] == [0, 1, 5]
    # output rows start at every 4-byte phase where newW * 3 is odd, at 0 and 2 where it is 2 mod 4
    assert [sorted({(r * c.new_w * 3) % 4 for r in range(c.n * c.h)}) for c in al] == [[0, 1, 2, 3], [0, 2], [0, 1, 2, 3], [0]]
    assert {(c.src_off + r * c.w * 3) % 16 for c in al for r in range(c.n * c.h)} == set(range(16))


def test_the_scale_cases_have_the_taps_they_are_chosen_for():
    from deepemia_amd.engine import pil_bilinear_tables
    by = {c.name: c for c in S.RESIZE_CASES}
    c = by["down-13-taps"]
    assert c.h / c.new_h > 2.56 and c.w / c.new_w > 2.56
    assert pil_bilinear_tables(c.h, c.new_h)[2].shape[1] == 13 == pil_bilinear_tables(c.w, c.new_w)[2].shape[1]
    assert int(pil_bilinear_tables(c.w, c.new_w)[1].max()) >= 12
    assert pil_bilinear_tables(200, 13)[2].shape[1] == 33
    assert pil_bilinear_tables(S.LDS_OVER, 1333)[2].shape[1] == 31
    assert pil_bilinear_tables(7, 18)[2].shape[1] == 3                   # upscale: at most three taps
    assert {c.content for c in S.RESIZE_CASES} == {"random", "zeros", "ones", "checker"}
    a, b = S.resize_images(by["lds-under"]), S.resize_images(by["lds-over"])
    assert np.array_equal(a, b[:, :, :S.LDS_UNDER])                      # the same content on both sides of the rule


# ---------------------------------------------------------------------------------------------------------------------
# Pillow
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_RESIZE, ids=lambda c: c.name)
def test_replay_of_both_passes_equals_pillow(case):
    imgs = S.resize_images(case)
    want = R.pillow_resize_u8(imgs, case.new_h, case.new_w)
    assert np.array_equal(R.pillow_replay(imgs, case.new_h, case.new_w), want)
    ref = R.pillow_reference(imgs, case.new_h, case.new_w)
    assert ref.dtype == np.float32 and ref.shape == (case.n, case.new_h, case.new_w, 3)
    assert not (ref == 0).any()                                            # no output value is a zero the border could hide


@pytest.mark.parametrize("sizes", S.REPLAY_SIZES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_replay_of_one_axis_equals_pillow(sizes):
    n_in, n_out = sizes
    rng = np.random.default_rng(n_in + n_out)
    row = rng.integers(0, 256, size=(1, 2, n_in, 3), dtype=np.uint8)
    assert np.array_equal(R.pillow_replay(row, 2, n_out), R.pillow_resize_u8(row, 2, n_out))
    col = np.ascontiguousarray(row.transpose(0, 2, 1, 3))
    assert np.array_equal(R.pillow_replay(col, n_out, 2), R.pillow_resize_u8(col, n_out, 2))


def test_the_rounding_constant_shows():
    """Dropping ``1 << 21`` from either pass changes bytes on the random cases, and on the all-255 image it turns 255 into 254
    wherever a table's coefficients sum to less than ``1 << 22``; the all-zero image cannot show it (that case is there for clip8)."""
    by = {c.name: c for c in S.RESIZE_CASES}
    for name in ("align-off0", "upscale", "down-13-taps", "same-h-300", "lds-over", "checker-down", "checker-up"):
        c = by[name]
        imgs = S.resize_images(c)
        assert not np.array_equal(R.pillow_replay(imgs, c.new_h, c.new_w, "pillow_no_rounding"), R.pillow_replay(imgs, c.new_h, c.new_w)), name
    c = by["ones-down"]
    imgs = S.resize_images(c)
    assert (R.pillow_replay(imgs, c.new_h, c.new_w) == 255).all()
    assert (R.pillow_replay(imgs, c.new_h, c.new_w, "pillow_no_rounding") == 254).any()


# ---------------------------------------------------------------------------------------------------------------------
# OpenCV INTER_LINEAR
# ---------------------------------------------------------------------------------------------------------------------
def test_linear_known_answers():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, size=(2, 7, 5, 3), dtype=np.uint8)
    assert np.array_equal(R.cv_linear_u8(img, 7, 5), img)                                 # same size: the identity
    for v in (0, 1, 127, 254, 255):
        const = np.full((1, 3, 4, 3), v, dtype=np.uint8)
        for oh, ow in [(6, 8), (5, 7), (2, 3), (1, 1), (3, 4)]:
            assert (R.cv_linear_u8(const, oh, ow) == v).all(), (v, oh, ow)
    # an exact 2x upscale of the ramp {0, 100, 200} over {+0, +40}: the weights are 512 / 1536 (a quarter and three quarters) or
    # 2048 on the border pixel, every product is a multiple of 65536, nothing is truncated:
    #   columns: 0, (3 * 0 + 100) / 4, (0 + 3 * 100) / 4, (3 * 100 + 200) / 4, (100 + 3 * 200) / 4, 200
    #   rows: +0, +10, +30, +40
    ramp = np.array([[0, 100, 200], [40, 140, 240]], dtype=np.uint8)[None, :, :, None].repeat(3, axis=3)
    want = np.array([0, 25, 75, 125, 175, 200])[None, :] + np.array([0, 10, 30, 40])[:, None]
    got = R.cv_linear_u8(ramp, 4, 6)
    assert np.array_equal(got[0, :, :, 0], want) and np.array_equal(got[0, :, :, 2], want)
    assert R._cv_axis(3, 6, False, None) == [(0, 1, 2048, 0), (0, 1, 1536, 512), (0, 1, 512, 1536), (1, 2, 1536, 512), (1, 2, 512, 1536), (2, 2, 2048, 0)]
    assert R._cv_axis(2, 4, True, None) == [(0, 0, 512, 1536), (0, 1, 1536, 512), (0, 1, 512, 1536), (1, 1, 1536, 512)]
    # factor 0.5: both fractions are one half, the result is the rounded mean of each 2 x 2 box
    img = rng.integers(0, 256, size=(1, 10, 14, 3), dtype=np.uint8)
    box = img.astype(np.int64).reshape(1, 5, 2, 7, 2, 3).sum(axis=(2, 4))
    assert np.array_equal(R.cv_linear_u8(img, 5, 7), (box + 2) >> 2)
    # coefficients round half to even: 2048 * 0.25024... is not a tie, but (1 - f) * 2048 = 0.5 exactly is
    assert R._cv_round_short(np.float32(0.5), False) == 0 and R._cv_round_short(np.float32(1.5), False) == 2
    assert R._cv_round_short(np.float32(0.5), True) == 1 and R._cv_round_short(np.float32(40000.0), False) == 32767


@pytest.mark.parametrize("case", S.LINEAR_CASES, ids=lambda c: c.name)
def test_linear_restatement_equals_the_oracle_and_the_engine_tables(case):
    from deepemia_amd.engine import cv_linear_tables
    from oracle.pipeline_ref import cv_resize_linear_u8

    imgs = S.linear_images(case)
    ref = R.cv_linear_u8(imgs, case.oh, case.ow)
    for i in range(case.n):
        assert np.array_equal(cv_resize_linear_u8(imgs[i], case.oh, case.ow), ref[i])
    for n_in, n_out, vertical in [(case.w, case.ow, False), (case.h, case.oh, True)]:
        ofs, coef = cv_linear_tables(n_in, n_out, vertical)
        mine = R._cv_axis(n_in, n_out, vertical, None)
        assert ofs.dtype == np.int32 and coef.dtype == np.int16
        assert [tuple(o) + tuple(c) for o, c in zip(ofs.tolist(), coef.tolist())] == mine


def test_the_case_list_of_the_linear_resize():
    cs = S.LINEAR_CASES
    pairs = {(c.w, c.ow) for c in cs} | {(c.h, c.oh) for c in cs}
    factors = {o / i for i, o in pairs}
    assert {2.0, 1.5, 0.75, 0.5} <= factors
    for p in [(37, 55), (101, 67), (5, 9)]:
        assert p in {(c.w, c.ow) for c in cs} and p in {(c.h, c.oh) for c in cs}, p
    assert {1, 2} <= {c.h for c in cs} and {1, 2} <= {c.w for c in cs}
    assert 1 in {c.oh for c in cs} and 1 in {c.ow for c in cs}
    assert any(c.h != c.w and c.oh != c.ow for c in cs) and any(c.n == 3 for c in cs)
    assert max(max(c.h, c.w, c.oh, c.ow) for c in cs) <= S.LINEAR_MAX_EXTENT


def test_the_two_edge_rules_differ_on_the_edge_rule_case():
    case = next(c for c in S.LINEAR_CASES if c.name == S.EDGE_RULE_CASE)
    assert (case.h, case.oh) == (case.w, case.ow)                     # the same extent pair on both axes
    imgs = S.linear_images(case)
    ref = R.cv_linear_u8(imgs, case.oh, case.ow)
    other = R.cv_linear_u8(imgs, case.oh, case.ow, "linear_h_rule_vertical")
    rows = sorted(set(np.nonzero(ref != other)[1].tolist()))
    assert rows and set(rows) <= {0, case.oh - 1}, rows              # only rows whose taps are clipped onto a border row can differ
    # the tables differ in those rows only: the fraction kept against the fraction zeroed
    v, h = R._cv_axis(case.h, case.oh, True, None), R._cv_axis(case.h, case.oh, True, "linear_h_rule_vertical")
    assert [i for i in range(case.oh) if v[i] != h[i]] == [0, case.oh - 1]
    assert h == R._cv_axis(case.w, case.ow, False, None)


def test_linear_distance_from_exact_bilinear_is_within_the_derived_bound():
    assert 1.26 < R.LINEAR_BOUND < 1.27
    worst = 0.0
    for case in S.LINEAR_CASES:
        imgs = S.linear_images(case)
        d = float(np.abs(R.cv_linear_u8(imgs, case.oh, case.ow).astype(np.float64) - R.exact_bilinear(imgs, case.oh, case.ow)).max())
        print(f"linear {case.name}: largest distance from exact bilinear {d:.4f} grey levels")
        worst = max(worst, d)
    print(f"largest over the cases: {worst:.4f}, derived bound {R.LINEAR_BOUND:.4f}")
    assert 0.5 < worst <= R.LINEAR_BOUND, worst                     # (a rounding to bytes alone reaches 0.5)
    recorded = float(re.search(r"over the cases: ([0-9.]+) grey levels", __doc__).group(1))
    assert abs(worst - recorded) < 5e-4, (worst, recorded)


@pytest.mark.parametrize("variant", ["linear_h_rule_vertical", "linear_round_half_up"])
def test_linear_variants_show(variant):
    hit = [c.name for c in S.LINEAR_CASES
           if not np.array_equal(R.cv_linear_u8(S.linear_images(c), c.oh, c.ow, variant), R.cv_linear_u8(S.linear_images(c), c.oh, c.ow))]
    print(variant, "changes bytes on", hit)
    assert hit, variant
    if variant == "linear_h_rule_vertical":
        assert S.EDGE_RULE_CASE in hit


def test_every_named_mistake_belongs_to_one_reference():
    takes = {"conv_pad2": R.stem_reference, "conv_phase": R.stem_reference, "pool_window_2o": R.pool_reference,
             "linear_h_rule_vertical": R.cv_linear_u8, "linear_round_half_up": R.cv_linear_u8, "pillow_no_rounding": R.pillow_replay}
    assert set(takes) == set(S.VARIANTS)
    with pytest.raises(AssertionError):
        R.pool_reference(torch.zeros((1, 4, 4, 4)), "conv_pad2")
    with pytest.raises(AssertionError):
        R.pillow_replay(np.zeros((1, 2, 2, 3), dtype=np.uint8), 3, 3, "linear_round_half_up")


# ---------------------------------------------------------------------------------------------------------------------
# stem and pools
# ---------------------------------------------------------------------------------------------------------------------
def test_pixel_mean_is_the_engines():
    from deepemia_amd import engine
    assert tuple(engine.PIXEL_MEAN) == S.PIXEL_MEAN


def test_the_stem_sizes_are_the_edges_they_are_chosen_for():
    """Conv tiles are 16 x 16 outputs (32 x 32 pixels); the fused kernel pools 7 x 7 outputs per workgroup."""
    conv = {(ph // 2, pw // 2) for ph, pw in S.STEM_SIZES}
    assert (16, 16) in conv                                               # exactly one tile
    assert any(h > 16 and w > 16 and (h % 16 == 0) for h, w in conv)      # several tiles
    pooled = {p // 4 for hw in S.STEM_SIZES for p in hw}
    assert pooled == {8, 16, 24, 40} and 8 % 7 == 1
    # smaller than one tile: the fused kernel's first tile covers conv rows -1 .. 14, so 16 conv rows leave its second tile with ONE
    # pooled row (7) whose window reaches conv rows 13 .. 15: a tile that holds two valid conv rows
    assert {c.n for c in S.STEM_CASES} == {1, 3} and len(S.STEM_CASES) == 10


@pytest.mark.parametrize("case", S.STEM_CASES, ids=lambda c: c.name)
def test_stem_operands_and_reference(case):
    ops = S.stem_operands(case)
    wt, scale, bias = ops["wt"], ops["scale"], ops["bias"]
    amax = wt.abs().flatten(1).amax(1)
    assert float(amax[S.ZERO_CHANNEL]) == 0
    nz = amax[amax > 0]
    assert float(nz.max() / nz.min()) > 300                              # magnitudes over (nearly) three decades
    assert int((scale < 0).sum()) >= 10
    ref = R.stem_reference(ops)
    assert ref.shape == (case.n, case.ph // 2, case.pw // 2, 64) and ref.dtype == torch.float64
    zeros = float((ref == 0).double().mean())
    assert 0.3 < zeros < 0.8, zeros                                       # many ReLU zeros, and many values that are not
    assert float(ref.max()) <= S.stem_bound(ops)
    x = R.stem_input(ops["bytes"])
    assert x.shape == (case.n, case.ph + 6, case.pw + 8, 4)
    assert not x[:, :3].any() and not x[:, case.ph + 3:].any() and not x[:, :, :3].any() and not x[:, :, case.pw + 3:].any() and not x[..., 3].any()
    # the reference of the unbordered interior is the plain convolution of the bordered tensor with no padding at all
    full = torch.nn.functional.conv2d(x[:, :, :case.pw + 6, :3].double().permute(0, 3, 1, 2), wt.double(), stride=2)
    full = torch.relu(full * scale.double().view(1, -1, 1, 1) + bias.double().view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    assert torch.equal(full, ref)
    # each deliberate mistake lies further than TELL x the bar from the reference, in the conv output and after the pool
    amax_ref = float(ref.abs().max())
    pooled = R.pool_reference(ref)
    for v in ("conv_pad2", "conv_phase"):
        wrong = R.stem_reference(ops, v)
        assert float((wrong - ref).abs().max()) / amax_ref > S.TELL * S.BAR, v
        assert float((R.pool_reference(wrong) - pooled).abs().max()) / float(pooled.abs().max()) > S.TELL * S.BAR, v
    wrong = R.pool_reference(ref, "pool_window_2o")
    assert wrong.shape == pooled.shape == (case.n, case.ph // 4, case.pw // 4, 64)
    assert float((wrong - pooled).abs().max()) / float(pooled.abs().max()) > S.TELL * S.BAR
    # an output right except for ONE element off by 3x the bar does not pass
    off = ref.clone()
    off[-1, -1, -1, -1] += 3 * S.BAR * amax_ref
    assert float((off - ref).abs().max()) / amax_ref > S.BAR


@pytest.mark.parametrize("case", S.POOL_P32_CASES + S.POOL_CASES, ids=lambda c: c.name)
def test_pool_reference_and_plane_split(case):
    x = S.pool_input(case)
    assert bool((x < 0).any()) and bool((x > 0).any())
    y = R.pool_reference(x)
    ho, wo = S.pooled_extent(case.h), S.pooled_extent(case.w)
    assert y.shape == (case.n, ho, wo, case.c)
    assert float(y.max()) < float(y.abs().max()) == -float(y[-1].min())          # the largest |pooled value| is a negative one
    # window 2 o - 1 .. 2 o + 1 clipped to the image, by hand
    for o_y, o_x in {(0, 0), (ho - 1, wo - 1), (ho // 2, wo // 2)}:
        win = x[:, max(2 * o_y - 1, 0):min(2 * o_y + 2, case.h), max(2 * o_x - 1, 0):min(2 * o_x + 2, case.w)]
        assert torch.equal(y[:, o_y, o_x], win.amax(dim=(1, 2)))
    if max(case.h, case.w) > 2:
        assert not torch.equal(R.pool_reference(x, "pool_window_2o"), y)
    if case.c % 32 == 0:
        from deepemia_amd import p32
        s = p32.plane_scale(float(x.abs().max()))
        for groups in {1, case.n}:
            planes, meta = R.p32_planes(y, s, groups, False)
            back = (planes[:, :, 0].float() + planes[:, :, 1].float()).reshape(y.shape) / s
            assert float((back - y).abs().max()) <= 2.0 ** -21 * float(y.abs().max())      # 22 significand bits
            assert float(planes.float().abs().max()) < 32768.0
            assert meta.shape == (groups, 2) and float(meta[:, 0].max()) == float(y.abs().max())
            one, _ = R.p32_planes(y, s, groups, True)
            assert torch.equal(one[:, :, 0], planes[:, :, 0]) and not one[:, :, 1].any() and planes[:, :, 1].any()
