"""The front end in two launches (``front_end_fused``): ``demia_resize_hv_u8x4`` and ``demia_stem_pool_mfma_u8`` against the
launches they replace, bit for bit, through the C ABI at edge sizes, and the engine with the switch on and off.

The new resize writes four bytes per pixel, (c0, c1, c2, flag), into a buffer that was zeroed once; the header's decoding rule
``x[c] = flag ? (float)c_c - mean[c] : 0``, ``x[3] = 0`` is restated here (``decode``) and must turn that buffer into the WHOLE f32
buffer of ``demia_resize_h_u8`` + ``demia_resize_v_norm`` (run on zeros): image, border, padding and fourth channel.  Cases and
tables come from ``front_end_cases.py`` / ``front_end_ref.py``; the f32 launches themselves are held to Pillow by
``test_gpu_front_end_edges.py``.

1. ``test_resize_hv_equals_the_two_launches``: the headline's 2.5625 ratio (205 -> 80, newW % 4 == 0), odd sizes with
   newW % 4 != 0, an upscale, W == newW (no horizontal pass), a padded size larger than the image in both axes, newH = 1, newH one
   less and one more than a strip (and a multiple), three images whose rows start at every byte alignment, strips chosen by the
   launch and given, 33 vertical taps.  The output lies between guards; what the launch leaves unwritten still holds the zeros.
2. ``test_resize_hv_at_the_lds_window``: the widest source row the kernel's LDS takes for 1333 output pixels, and the next one: the
   entry refuses it and writes nothing, ``demia_resize_hv_fits`` says so beforehand.
3. ``test_stem_u8_equals_the_f32_stem``: ``demia_stem_pool_mfma_u8`` on ``STEM_CASES`` (image smaller than the padded size, random
   bytes under flag 0 in border and padding) against ``demia_stem_pool_mfma`` on the decoded buffer: planes and meta equal for
   groups 1 and N, single 0 and 1.  That the comparison can fail: the f32 stem on a buffer decoded with ONE mistake (``wrong_mean``:
   the means of channels 0 and 2 swapped; ``flag_ignored``: border bytes decoded as pixels) gives other planes.
4. ``test_engine_front_end_fused_on_and_off``: R50, two 256 x 256 tiles, eager and graph replay: identical ``RawDetections``
   (``valid`` and ``count`` whole; the rows below ``count`` of the others -- the rows behind are never written), an f32 ``dbg["xin"]``
   either way; the widest 512-row image whose rows fit the resize kernel's LDS runs fused, one pixel more takes ``preprocess``.

MEASURED on an MI355X with the product library: 35 passed in 2.3 s (the engine test 0.7 s, the first launch 0.65 s, every other test
under 0.1 s); no difference in any case.  A first version of the resize kernel's tap loop and two later ones gave the same bytes.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import front_end_cases as S
import front_end_ref as R

pytestmark = pytest.mark.gpu

CANARY8 = 0xA5
CANARY16 = 0x7BCD
CANARY32 = 0x7FC0BEEF
GUARD = 256
DECODE_VARIANTS = ("wrong_mean", "flag_ignored")


@pytest.fixture(scope="module")
def env(gpu_device):
    from deepemia_amd import _lib
    e = SimpleNamespace(dev=gpu_device, lib=_lib.load(), cache={})
    yield e
    e.cache.clear()


def stream() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def guarded(dev, numel: int, dtype, canary: int):
    whole = torch.full((numel + 2 * GUARD,), canary, dtype=dtype, device=dev)
    assert whole.data_ptr() % 16 == 0
    return whole, whole[GUARD:GUARD + numel]


def guards_intact(whole, canary: int) -> bool:
    return bool((whole[:GUARD] == canary).all()) and bool((whole[-GUARD:] == canary).all())


def decode(buf: torch.Tensor, variant=None) -> torch.Tensor:
    """[..., 4] u8 (c0, c1, c2, flag) -> [..., 4] f32 by the rule of ``include/deepemia_hip.h``, or with one deliberate mistake."""
    assert variant is None or variant in DECODE_VARIANTS
    mean = S.PIXEL_MEAN if variant != "wrong_mean" else S.PIXEL_MEAN[::-1]
    mean = torch.tensor(mean, dtype=torch.float32, device=buf.device)
    x = torch.zeros(buf.shape, dtype=torch.float32, device=buf.device)
    val = buf[..., :3].to(torch.float32) - mean
    x[..., :3] = val if variant == "flag_ignored" else torch.where(buf[..., 3:] != 0, val, torch.zeros_like(val))
    return x


def pil_tables(env, n_in, n_out):
    key = ("pil", n_in, n_out)
    if key not in env.cache:
        from deepemia_amd.engine import pil_bilinear_tables
        lo, cnt, k = pil_bilinear_tables(n_in, n_out)
        env.cache[key] = (torch.from_numpy(lo).to(env.dev), torch.from_numpy(cnt).to(env.dev), torch.from_numpy(k).to(env.dev), int(k.shape[1]))
    return env.cache[key]


def source_on_device(env, case, imgs):
    nbytes = imgs.size
    g = torch.Generator().manual_seed(nbytes)
    around = torch.randint(0, 256, (16 + nbytes + 64,), generator=g, dtype=torch.uint8).to(env.dev)
    assert around.data_ptr() % 16 == 0
    around[case.src_off:case.src_off + nbytes] = torch.from_numpy(imgs).reshape(-1).to(env.dev)
    return around


def two_launches(env, case, around):
    """The f32 stem input [n, PH + 6, PW + 8, 4] of the two existing launches, written into zeros."""
    from deepemia_amd import _lib
    lib, dev = env.lib, env.dev
    n, h, w, nh, nw = case.n, case.h, case.w, case.new_h, case.new_w
    src = _lib.ptr(around) + case.src_off
    if w != nw:
        xm, xs, xk, ksx = pil_tables(env, w, nw)
        tmp = torch.empty((n * h * nw * 3,), dtype=torch.uint8, device=dev)
        _lib.check(lib.demia_resize_h_u8(src, _lib.ptr(tmp), n, h, w, nw, _lib.ptr(xm), _lib.ptr(xs), _lib.ptr(xk), ksx, stream()), "demia_resize_h_u8")
        tmp_ptr = _lib.ptr(tmp)
    else:
        tmp_ptr = src
    ym, ys, yk, ksy = pil_tables(env, h, nh)
    dst = torch.zeros((n, case.ph + 6, case.pw + 8, 4), dtype=torch.float32, device=dev)
    mean = (C.c_float * 3)(*S.PIXEL_MEAN)
    _lib.check(lib.demia_resize_v_norm(tmp_ptr, _lib.ptr(dst), n, h, nw, nh, case.ph, case.pw, _lib.ptr(ym), _lib.ptr(ys), _lib.ptr(yk), ksy, mean,
                                       _lib.F32, stream()), "demia_resize_v_norm")
    torch.cuda.synchronize()
    return dst


def one_launch(env, case, around, strip):
    """(status, whole, body [n, PH + 6, PW + 8, 4] u8) of ``demia_resize_hv_u8x4`` into zeros between guards."""
    from deepemia_amd import _lib
    n, h, w, nh, nw = case.n, case.h, case.w, case.new_h, case.new_w
    null = torch.empty((0,), dtype=torch.int32, device=env.dev)
    xm, xs, xk, ksx = pil_tables(env, w, nw) if w != nw else (null, null, null, 0)
    ym, ys, yk, ksy = pil_tables(env, h, nh)
    whole, body = guarded(env.dev, n * (case.ph + 6) * (case.pw + 8) * 4, torch.uint8, CANARY8)
    body.zero_()
    status = env.lib.demia_resize_hv_u8x4(_lib.ptr(around) + case.src_off, _lib.ptr(body), n, h, w, nh, nw, case.ph, case.pw,
                                          _lib.ptr(xm) if w != nw else None, _lib.ptr(xs) if w != nw else None, _lib.ptr(xk) if w != nw else None,
                                          ksx, _lib.ptr(ym), _lib.ptr(ys), _lib.ptr(yk), ksy, strip, stream())
    torch.cuda.synchronize()
    return status, whole, body.view(n, case.ph + 6, case.pw + 8, 4)


# (case, strip): strip 0 = chosen by the launch (8 .. 32 rows)
HV_CASES = [
    (S.ResizeCase("headline-ratio", 2, 205, 205, 80, 80), 0),
    (S.ResizeCase("headline-ratio-strip8", 2, 205, 205, 80, 80, src_off=1), 8),
    (S.ResizeCase("odd-37x53", 2, 37, 53, 13, 19, src_off=5), 0),
    (S.ResizeCase("odd-37x53-strip3", 2, 37, 53, 13, 19, src_off=5), 3),
    (S.ResizeCase("upscale", 2, 5, 7, 13, 18), 0),
    (S.ResizeCase("upscale-strip2", 2, 5, 7, 13, 18, src_off=15), 2),
    (S.ResizeCase("same-w-36", 2, 41, 36, 30, 36), 0),
    (S.ResizeCase("same-w-37-off1", 3, 41, 37, 30, 37, src_off=1), 8),
    (S.ResizeCase("identity-both", 3, 9, 12, 9, 12, src_off=5), 0),
    (S.ResizeCase("padded-both-axes", 1, 50, 70, 33, 40), 0),
    (S.ResizeCase("new-h-1", 2, 9, 12, 1, 5, src_off=1), 0),
    (S.ResizeCase("in1-out1", 1, 1, 1, 1, 1), 0),
    (S.ResizeCase("strip-minus-1", 2, 23, 50, 7, 36), 8),
    (S.ResizeCase("strip-exact", 2, 23, 50, 8, 36), 8),
    (S.ResizeCase("strip-plus-1", 2, 23, 50, 9, 36, src_off=1), 8),
    (S.ResizeCase("strip-x2-plus-1", 2, 23, 50, 17, 36), 8),
    (S.ResizeCase("align-off0", 3, 5, 37, 4, 21, src_off=0), 0),
    (S.ResizeCase("align-off1", 3, 5, 37, 3, 22, src_off=1), 0),
    (S.ResizeCase("align-off15", 3, 5, 37, 2, 20, src_off=15), 1),
    (S.ResizeCase("down-200-13", 2, 200, 200, 13, 13, src_off=1), 0),          # 33 taps: a ring of 33 rows
    (S.ResizeCase("moderate-4100", 2, 3, 4100, 3, 800, src_off=1), 0),         # 12.3 KB rows: chunks behind the two register ones
    (S.ResizeCase("ones-down", 2, 23, 37, 9, 14, content="ones"), 0),
    (S.ResizeCase("checker-up", 2, 6, 5, 15, 13, content="checker"), 0),
]


@pytest.mark.parametrize("case,strip", HV_CASES, ids=[c.name for c, _ in HV_CASES])
def test_resize_hv_equals_the_two_launches(env, case, strip):
    assert (case.w * 3) % 16 != 0 or not case.name.startswith("align")
    around = source_on_device(env, case, S.resize_images(case))
    want = two_launches(env, case, around)
    lds = int(env.lib.demia_resize_hv_fits(case.w, case.new_w, pil_tables(env, case.h, case.new_h)[3]))
    print(f"{case.name}: N = {case.n}, {case.h} x {case.w} -> {case.new_h} x {case.new_w} in {case.ph} x {case.pw}, source at +{case.src_off}, strip {strip}, LDS {lds} B")
    assert lds > 0
    status, whole, got = one_launch(env, case, around, strip)
    assert status == 0 and guards_intact(whole, CANARY8)
    dec = decode(got)
    if not torch.equal(dec.view(torch.int32), want.view(torch.int32)):
        bad = (dec.view(torch.int32) != want.view(torch.int32)).nonzero()
        pytest.fail(f"{case.name}: {bad.shape[0]} words differ, first (n, y, x, c) = {bad[:6].tolist()}")
    # the bytes themselves: (c0, c1, c2, 1) inside the image, untouched zeros everywhere else
    inside = torch.zeros(got.shape[:3], dtype=torch.bool, device=env.dev)
    inside[:, 3:3 + case.new_h, 3:3 + case.new_w] = True
    assert bool((got[..., 3] == inside.to(torch.uint8)).all()) and not bool(got[~inside].any())
    # a wrong mean or an ignored flag in the decoding would not have passed
    assert not torch.equal(decode(got, "wrong_mean"), want)
    got[:, 0, 0, 0] = 7                                                     # a stale byte in the border, flag 0
    assert torch.equal(decode(got), want) and not torch.equal(decode(got, "flag_ignored"), want)


def test_resize_hv_at_the_lds_window(env):
    """1333 output pixels, three rows, one vertical tap: the widest source row whose staging buffer and ring fit, and the next."""
    new_w, h = 1333, 3
    ksy = pil_tables(env, h, h)[3]
    fits = lambda w: int(env.lib.demia_resize_hv_fits(w, new_w, ksy))
    w = 8192
    assert fits(w) > 0
    while fits(w + 1024) > 0:
        w += 1024
    while fits(w + 1) > 0:
        w += 1
    assert 0 < fits(w) <= 60 * 1024 and fits(w + 1) == 0
    under = S.ResizeCase("hv-lds-under", 1, h, w, h, new_w, gen_w=w + 1)
    over = S.ResizeCase("hv-lds-over", 1, h, w + 1, h, new_w, src_off=1, gen_w=w + 1)
    print(f"widest row: {w} pixels, LDS {fits(w)} B, ksy {ksy}")
    around = source_on_device(env, under, S.resize_images(under))
    status, whole, got = one_launch(env, under, around, 0)
    assert status == 0 and guards_intact(whole, CANARY8)
    assert torch.equal(decode(got).view(torch.int32), two_launches(env, under, around).view(torch.int32))
    around = source_on_device(env, over, S.resize_images(over))
    status, whole, got = one_launch(env, over, around, 0)
    assert status != 0 and guards_intact(whole, CANARY8) and not bool(got.any())
    assert b"LDS" in env.lib.demia_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the stem on bytes
# ---------------------------------------------------------------------------------------------------------------------
def p32_buffer(dev, pixels, channels):
    whole, body = guarded(dev, 64 + 2 * pixels * channels, torch.int16, CANARY16)
    body[:64] = 0
    return whole, body


def meta_buffer(dev, groups):
    whole, body = guarded(dev, 2 * groups, torch.int32, CANARY32)
    body.zero_()
    return whole, body


def stem_state(env, case):
    key = ("stem-u8", case)
    if key not in env.cache:
        from deepemia_amd import engine as E
        from deepemia_amd import p32
        ops = S.stem_operands(case)
        n, ph, pw = case.n, case.ph, case.pw
        nh, nw = ph - 5, pw - 3                                            # the image is smaller than the padded size
        g = torch.Generator().manual_seed(5000 + ph + pw)
        buf = torch.randint(0, 256, (n, ph + 6, pw + 8, 4), generator=g, dtype=torch.uint8)   # stale bytes everywhere ...
        buf[..., 3] = 0                                                                        # ... under flag 0
        buf[:, 3:3 + nh, 3:3 + nw, :3] = ops["bytes"][:, :nh, :nw]
        buf[:, 3:3 + nh, 3:3 + nw, 3] = 1
        planes, sw = E.stem_weight_planes(ops["wt"])
        s_in = p32.plane_scale(255.0 - min(S.PIXEL_MEAN))
        env.cache[key] = SimpleNamespace(
            buf=buf.to(env.dev), planes=planes.to(env.dev).contiguous(), scale_mfma=(ops["scale"] / (sw * s_in)).to(env.dev).contiguous(),
            bias=ops["bias"].to(env.dev), s_in=s_in, s_out=p32.plane_scale(S.stem_bound(ops)))
    return env.cache[key]


def stem_f32(env, st, case, xin, groups, single):
    from deepemia_amd import _lib
    pixels = case.n * (case.ph // 4) * (case.pw // 4)
    whole, out = p32_buffer(env.dev, pixels, 64)
    mw, meta = meta_buffer(env.dev, groups)
    _lib.check(env.lib.demia_stem_pool_mfma(_lib.ptr(xin), _lib.ptr(st.planes), _lib.ptr(st.scale_mfma), _lib.ptr(st.bias), _lib.ptr(out), _lib.ptr(meta),
                                            case.n, case.ph, case.pw, st.s_in, st.s_out, groups, single, stream()), "demia_stem_pool_mfma")
    torch.cuda.synchronize()
    assert guards_intact(whole, CANARY16) and guards_intact(mw, CANARY32)
    return out, meta


@pytest.mark.parametrize("case", S.STEM_CASES, ids=lambda c: c.name)
def test_stem_u8_equals_the_f32_stem(env, case):
    from deepemia_amd import _lib
    st = stem_state(env, case)
    pixels = case.n * (case.ph // 4) * (case.pw // 4)
    xin = decode(st.buf).contiguous()
    mean = (C.c_float * 3)(*S.PIXEL_MEAN)
    for groups in sorted({1, case.n}):
        for single in (0, 1):
            what = f"{case.name}, groups = {groups}, single = {single}"
            want, want_meta = stem_f32(env, st, case, xin, groups, single)
            whole, out = p32_buffer(env.dev, pixels, 64)
            mw, meta = meta_buffer(env.dev, groups)
            _lib.check(env.lib.demia_stem_pool_mfma_u8(_lib.ptr(st.buf), mean, _lib.ptr(st.planes), _lib.ptr(st.scale_mfma), _lib.ptr(st.bias), _lib.ptr(out),
                                                       _lib.ptr(meta), case.n, case.ph, case.pw, st.s_in, st.s_out, groups, single, stream()),
                       "demia_stem_pool_mfma_u8")
            torch.cuda.synchronize()
            assert guards_intact(whole, CANARY16) and guards_intact(mw, CANARY32), what
            assert torch.equal(out, want), (what, f"{int((out != want).sum())} of {out.numel()} halfs differ")
            assert torch.equal(meta, want_meta), (what, meta.view(torch.float32).tolist(), want_meta.view(torch.float32).tolist())
            assert bool(out[64:].any()) and float(meta.view(torch.float32)[0]) > 0
    # the comparison can fail: one mistake in the decoding moves the planes of the f32 stem
    base, _ = stem_f32(env, st, case, xin, 1, 0)
    for variant in DECODE_VARIANTS:
        other, _ = stem_f32(env, st, case, decode(st.buf, variant).contiguous(), 1, 0)
        assert not torch.equal(other, base), variant


# ---------------------------------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------------------------------
def outputs_of(raw):
    """``valid`` and ``count`` whole; of the other tensors the rows below ``count`` (the rows behind them are never written)."""
    out = [raw.height, raw.width, raw.valid.clone(), raw.count.clone()]
    for i, c in enumerate(raw.count.tolist()):
        out += [t[i, :c].clone() for t in (raw.boxes, raw.scores, raw.classes, raw.packed, raw.bbox)]
    return out


def same(a, b) -> bool:
    return len(a) == len(b) and all(x == y if isinstance(x, int) else torch.equal(x, y) for x, y in zip(a, b))


def test_engine_front_end_fused_on_and_off(gpu_device):
    from deepemia_amd import synth
    from deepemia_amd.engine import MaskRCNNEngine
    sd = synth.random_d2_state_dict(50, 2, seed=0)
    on = MaskRCNNEngine(sd, 50, 2, 0.3, gpu_device, "f16x2")
    off = MaskRCNNEngine(sd, 50, 2, 0.3, gpu_device, "f16x2")
    assert on.front_end_fused
    off.front_end_fused = False
    calls = []
    on_preprocess = on.preprocess
    on.preprocess = lambda images: (calls.append(tuple(images.shape)), on_preprocess(images))[1]
    imgs = torch.from_numpy(np.stack([synth.em_tile(7, 256), synth.em_tile(8, 256)])).to(gpu_device)
    assert on.front_end_fits(256, 256) and not off.front_end_fits(256, 256)
    a = on.forward(imgs, keep_intermediates=True)
    b = off.forward(imgs, keep_intermediates=True)
    torch.cuda.synchronize()
    assert not calls, "the fused front end went through preprocess"
    assert a.dbg["xin"].dtype == torch.float32 and torch.equal(a.dbg["xin"].view(torch.int32), b.dbg["xin"].view(torch.int32))
    assert torch.equal(a.dbg["feats"]["stem"].buf, b.dbg["feats"]["stem"].buf)
    want = outputs_of(b)
    assert sum(b.count.tolist()) > 0 and same(outputs_of(a), want)
    for eng in (on, off):
        eng.forward_graphed(imgs)
        replay = eng.forward_graphed(imgs)                     # the second slot's graph
        torch.cuda.synchronize()
        assert same(outputs_of(replay), want)
    assert not calls
    # the widest 512-row image whose rows still fit the resize kernel's LDS, and one pixel more: there the engine keeps the two launches
    from deepemia_amd.engine import pil_bilinear_tables, resize_shape
    h = 512

    def fits(w):
        newh, neww = resize_shape(h, w, on.min_size_test, on.max_size_test)
        return int(on.lib.demia_resize_hv_fits(w, neww, pil_bilinear_tables(h, newh)[2].shape[1])) > 0

    assert fits(2048) and not fits(8192)
    w = max(w for w in range(2048, 8192) if fits(w))
    print(f"widest 512-row image of the fused front end: {w} pixels")
    rng = np.random.default_rng(3)
    for width, fused in ((w, True), (w + 1, False)):
        assert on.front_end_fits(h, width) == fused and not off.front_end_fits(h, width)
        wide = torch.from_numpy(rng.integers(0, 256, size=(1, h, width, 3), dtype=np.uint8)).to(gpu_device)
        del calls[:]
        a = on.forward(wide)
        b = off.forward(wide)
        torch.cuda.synchronize()
        assert calls == ([] if fused else [(1, h, width, 3)]), (width, calls)
        assert same(outputs_of(a), outputs_of(b)), width
    on.release_cached_shapes()
    off.release_cached_shapes()
