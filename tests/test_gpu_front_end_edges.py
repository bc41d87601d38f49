"""The ten kernels of ``csrc/preproc_stem.hip`` at edge sizes, through the C ABI, against exact and float64 references.

Everything is called as ``_lib.check(lib.demia_...)`` on caller-owned buffers at tiny shapes, from tables made on the host.
Every output buffer lies between two guards of a recognisable pattern (``0xA5`` bytes, fp16 ``0x7BCD``, the f32 NaN payload
``0x7FC0BEEF``) that must survive every launch.  Cases and kernel rules: ``front_end_cases.py``; references:
``front_end_ref.py``; both are checked without a GPU by ``test_cpu_front_end_ref.py``.

1. ``test_resize_*``: ``demia_resize_h_u8`` + ``demia_resize_v_norm`` against Pillow itself, bit for bit.  ``dst`` is filled with
   the NaN payload before the launch and compared WHOLE with what it must hold afterwards: Pillow's bytes minus the mean
   inside the image, 0 in its fourth channel, the payload everywhere else -- border and padding are never written, which
   is what the zero-once arena buffer of the f16x2 path relies on (``test_preprocess_into_a_reused_arena_buffer`` runs that
   path itself).  The source sits at byte offsets 0, 1, 5 and 15 of a buffer of random bytes.  Kernels reached
   (horizontal / vertical; ``none`` = the width does not change and ``tmp`` is the source):

     lds-under row/norm, lds-over plain/norm, wide-20000 plain/norm, moderate-4100 row/norm4, align-off0 row/norm,
     align-off1 row/norm, align-off5 row/norm, align-off15 row/norm4, align-up-off15 row/norm, upscale row/norm,
     down-13-taps row/norm, down-200-13 row/norm, in1-out1 none/norm, in1-out5 row/norm, in2x3-out1 row/norm,
     same-w-1333 none/norm, same-w-36 none/norm4, same-h-300 row/norm, same-w-300 none/norm (misaligned source),
     identity-both none/norm, zeros-/ones-/checker-down row/norm, zeros-/ones-/checker-up row/norm, checker-wide plain/norm,
     v-mod1..3 row/norm, v-pair row/norm4 and, with DEMIA_RESIZE_PLAIN=1 or ``tmp`` moved on by one byte, row/norm.

   lds-under and lds-over are the widest source row that still takes ``resize_h_row_kernel`` for 1333 output pixels
   (19130) and the next one, cut from the same random image.
2. ``test_resize_linear_*``: ``demia_resize_linear_u8`` from ``engine.cv_linear_tables`` against the scalar restatement of
   OpenCV's fixed-point path, bit for bit.  The restatement lies at most 0.7758 grey levels from exact float64 bilinear
   interpolation over these cases (derived bound 1.264: ``front_end_ref.py``).
3. ``test_stem_*``, ``test_maxpool_*``, ``test_subsample2_*``: the f32 stem, the stem on the matrix pipe and the fused stem + pool
   against float64 ``relu(conv2d * scale + bias)`` and ``max_pool2d`` at padded sizes 32 x 32 .. 96 x 160 (less than a tile,
   one tile, several; pooled extents 8 = 7 + 1, 16, 24, 40), the allocation around the input filled with NaN; the fused
   kernel equal to the two-kernel path bit for bit; the P32 pool against a torch restatement of the plane split; the plain
   pool and the P6 subsample exact in f32 and bf16.  With ``single = 1`` the low plane is zero by contract, so the decoded
   tensor carries fp16's 11 bits and cannot meet an f32-sized bar: the f64 bar is applied to ``single = 0``, and
   ``single = 1`` must give the SAME high plane with an all-zero low plane.

MEASURED on an MI355X with the product library: 91 passed, no kernel or table bug found.  Every resize case gives
Pillow's bytes through the kernels listed above and leaves border, padding, guards and ``tmp``'s guards alone; the two
vertical kernels agree bit for bit; the linear resize equals the restatement on every case.  Largest error against f64
over the stem cases, as a fraction of max |reference| (bar 2e-5): ``demia_stem_conv`` f32 4.9e-7 (64x96-n1),
``demia_stem_conv_mfma`` 3.5e-7 (32x32), fused ``demia_stem_pool_mfma`` decoded 3.7e-7 (96x160-n3); fused and two-kernel
planes and meta identical for every groups / single combination.  Wall time of the module: 2.1 s (the engine-level
test 0.7 s, the first launch 0.6 s, every other test under 0.05 s).

That the tests can fail was checked once against a build with ONE deliberate arithmetic mistake per kernel (addressing
untouched): a halved rounding constant in ``resize_h_kernel``, the last tail byte of ``resize_h_row_kernel`` not stored, a
fourth channel of 1 in ``resize_v_norm_kernel``, the wrong mean in ``resize_v_norm4_kernel``, ``+ 1`` for ``+ 2`` in the linear
resize, a ReLU threshold of 1e-3 in ``stem_conv_kernel``, the a_l b_h product dropped in ``stem_mfma_kernel``, positions outside
the image not zeroed in the fused kernel, max for max |x| in the P32 pool, 0 for -inf in the plain pool, odd rows in the
subsample.  83 of the 91 tests failed, tests of every kernel among them.  The eight that passed cannot see their kernel's
mistake: the linear resize of a one-pixel-wide or one-pixel-high source, and six f32 stem cases without an output
between 0 and the bar.  (A first version of the pool inputs let the P32 pool's mistake through: the largest |pooled
value| was always positive.  ``front_end_cases.pool_input`` now makes it a negative one.)
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
CANARY16 = 0x7BCD            # fp16 bit pattern
CANARY32 = 0x7FC0BEEF        # f32 bit pattern (a NaN payload)
GUARD = 256                  # elements on either side of a buffer


@pytest.fixture(scope="module")
def env(gpu_device):
    from deepemia_amd import _lib
    e = SimpleNamespace(dev=gpu_device, lib=_lib.load(), cache={})
    yield e
    e.cache.clear()


def stream() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def guarded(dev, numel: int, dtype, canary: int):
    """(whole, body): ``numel`` elements between two guards, everything filled with ``canary``.  The body starts on a multiple of 256 bytes."""
    whole = torch.full((numel + 2 * GUARD,), canary, dtype=dtype, device=dev)
    assert whole.data_ptr() % 16 == 0
    return whole, whole[GUARD:GUARD + numel]


def guards_intact(whole, canary: int) -> bool:
    return bool((whole[:GUARD] == canary).all()) and bool((whole[-GUARD:] == canary).all())


def describe_difference(a, b):
    d = (a != b).nonzero().flatten()
    return f"{d.numel()} of {a.numel()} elements differ, first at {d[:6].tolist()}"


# ---------------------------------------------------------------------------------------------------------------------
# 1. Pillow-exact resize
# ---------------------------------------------------------------------------------------------------------------------
def pil_tables(env, n_in, n_out):
    key = ("pil", n_in, n_out)
    if key not in env.cache:
        from deepemia_amd.engine import pil_bilinear_tables
        lo, cnt, k = pil_bilinear_tables(n_in, n_out)
        env.cache[key] = (torch.from_numpy(lo).to(env.dev), torch.from_numpy(cnt).to(env.dev), torch.from_numpy(k).to(env.dev), int(k.shape[1]))
    return env.cache[key]


def run_resize(env, case, imgs, tmp_shift=0):
    """Both passes of one case.  Returns (dst whole buffer as int32, what it must equal, tmp guards intact)."""
    from deepemia_amd import _lib
    dev, lib = env.dev, env.lib
    n, h, w, nh, nw = case.n, case.h, case.w, case.new_h, case.new_w
    nbytes = imgs.size
    g = torch.Generator().manual_seed(nbytes)
    around = torch.randint(0, 256, (16 + nbytes + 64,), generator=g, dtype=torch.uint8).to(dev)
    assert around.data_ptr() % 16 == 0
    around[case.src_off:case.src_off + nbytes] = torch.from_numpy(imgs).reshape(-1).to(dev)
    src = _lib.ptr(around) + case.src_off
    tmp_ok = True
    moved_whole = None
    if w != nw:
        xm, xs, xk, ksx = pil_tables(env, w, nw)
        tmp_whole, tmp = guarded(dev, n * h * nw * 3, torch.uint8, CANARY8)
        _lib.check(lib.demia_resize_h_u8(src, _lib.ptr(tmp), n, h, w, nw, _lib.ptr(xm), _lib.ptr(xs), _lib.ptr(xk), ksx, stream()), "demia_resize_h_u8")
        torch.cuda.synchronize()
        tmp_ok = guards_intact(tmp_whole, CANARY8)
        tmp_ptr = _lib.ptr(tmp)
        if tmp_shift:
            moved_whole, moved = guarded(dev, n * h * nw * 3 + tmp_shift, torch.uint8, CANARY8)
            moved[tmp_shift:] = tmp
            tmp_ptr = _lib.ptr(moved) + tmp_shift
    else:
        assert tmp_shift == 0
        tmp_ptr = src
    ym, ys, yk, ksy = pil_tables(env, h, nh)
    ph, pw = case.ph, case.pw
    dst_whole, dst = guarded(dev, n * (ph + 6) * (pw + 8) * 4, torch.int32, CANARY32)
    want_whole = dst_whole.clone()
    mean = (C.c_float * 3)(*S.PIXEL_MEAN)
    _lib.check(lib.demia_resize_v_norm(tmp_ptr, _lib.ptr(dst), n, h, nw, nh, ph, pw, _lib.ptr(ym), _lib.ptr(ys), _lib.ptr(yk), ksy, mean,
                                       _lib.F32, stream()), "demia_resize_v_norm")
    torch.cuda.synchronize()
    if moved_whole is not None:
        tmp_ok = tmp_ok and guards_intact(moved_whole, CANARY8)
    ref = torch.from_numpy(R.pillow_reference(imgs, nh, nw)).view(torch.int32).to(dev)
    inside = want_whole[GUARD:-GUARD].view(n, ph + 6, pw + 8, 4)[:, 3:3 + nh, 3:3 + nw]
    inside[..., :3] = ref
    inside[..., 3] = 0
    return dst_whole, want_whole, tmp_ok


def assert_resize(case, got, want, tmp_ok):
    assert tmp_ok, "a guard of tmp was written"
    if not torch.equal(got, want):
        n_, dh, dw = case.n, case.ph + 6, case.pw + 8
        body = (got[GUARD:-GUARD] != want[GUARD:-GUARD]).view(n_, dh, dw, 4).nonzero()
        pytest.fail(f"{case.name}: guards intact = {guards_intact(got, CANARY32)}; {body.shape[0]} words of dst differ, first (n, y, x, c) = {body[:6].tolist()}")


@pytest.mark.parametrize("case", S.RESIZE_CASES + S.V_MOD, ids=lambda c: c.name)
def test_resize_bit_exact_vs_pillow(env, case):
    print(f"{case.name}: N = {case.n}, {case.h} x {case.w} -> {case.new_h} x {case.new_w}, source at +{case.src_off}: horizontal {case.hk}, vertical {case.vk}")
    got, want, tmp_ok = run_resize(env, case, S.resize_images(case))
    assert_resize(case, got, want, tmp_ok)


def test_resize_both_vertical_kernels_on_the_same_input(env, monkeypatch):
    """newW % 4 == 0: the four-pixel kernel, the plain one under DEMIA_RESIZE_PLAIN=1 (read by ``getenv`` on every call), and the
    plain one again because ``tmp`` starts one byte off a dword: the same ``dst``, which is Pillow's."""
    case = S.V_PAIR
    assert case.vk == "norm4"
    imgs = S.resize_images(case)
    four, want, ok = run_resize(env, case, imgs)
    assert_resize(case, four, want, ok)
    monkeypatch.setenv("DEMIA_RESIZE_PLAIN", "1")
    plain, _, ok = run_resize(env, case, imgs)
    monkeypatch.delenv("DEMIA_RESIZE_PLAIN")
    assert_resize(case, plain, want, ok)
    moved, _, ok = run_resize(env, case, imgs, tmp_shift=1)
    assert_resize(case, moved, want, ok)
    assert torch.equal(four, plain) and torch.equal(four, moved)


def test_preprocess_into_a_reused_arena_buffer(env):
    """The f16x2 engine writes the stem input into an arena buffer that is zeroed ONCE, when the shape is first seen.  Three
    images of one shape, then other shapes, then the first shape again: each result equals the f32 engine's (a fresh zero
    buffer per call) bit for bit, border and padding included.  Shapes with newW = 1319 (plain vertical kernel) and 800
    (four pixels per thread)."""
    from deepemia_amd import synth
    from deepemia_amd.engine import MaskRCNNEngine

    sd = synth.random_d2_state_dict(50, 2, seed=0)
    e32 = MaskRCNNEngine(sd, 50, 2, 0.3, env.dev, "f32")
    e16 = MaskRCNNEngine(sd, 50, 2, 0.3, env.dev, "f16x2")
    rng = np.random.default_rng(77)
    ptrs = {}

    def check(shape, content):
        imgs = rng.integers(0, 256, size=shape + (3,), dtype=np.uint8)
        if content == "dark":
            imgs //= 5
        elif content == "white":
            imgs[:] = 255
        x = torch.from_numpy(imgs).to(env.dev)
        want = e32.preprocess(x)
        got = e16.preprocess(x)
        torch.cuda.synchronize()
        assert got[1:] == want[1:]
        assert got[0].shape == want[0].shape
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), (shape, content, describe_difference(got[0], want[0]))
        assert ptrs.setdefault(shape, got[0].data_ptr()) == got[0].data_ptr(), "the arena buffer of this shape was not reused"

    a, b, c = (2, 37, 61), (1, 61, 37), (2, 50, 50)
    for content in ("random", "dark", "white"):
        check(a, content)
    for content in ("white", "random", "dark"):
        check(c, content)
    check(b, "random")
    check(a, "random")
    check(c, "white")
    check(a, "dark")
    e16.release_cached_shapes()


# ---------------------------------------------------------------------------------------------------------------------
# 2. OpenCV INTER_LINEAR
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", S.LINEAR_CASES, ids=lambda c: c.name)
def test_resize_linear_bit_exact_vs_the_restatement(env, case):
    from deepemia_amd import _lib
    from deepemia_amd.engine import cv_linear_tables

    imgs = S.linear_images(case)
    want = torch.from_numpy(R.cv_linear_u8(imgs, case.oh, case.ow)).to(env.dev)
    xo, xa = cv_linear_tables(case.w, case.ow)
    yo, ya = cv_linear_tables(case.h, case.oh, vertical=True)
    xo, xa, yo, ya = (torch.from_numpy(t).to(env.dev) for t in (xo, xa, yo, ya))
    src = torch.from_numpy(imgs).to(env.dev)
    whole, dst = guarded(env.dev, want.numel(), torch.uint8, CANARY8)
    _lib.check(env.lib.demia_resize_linear_u8(_lib.ptr(src), _lib.ptr(dst), case.n, case.h, case.w, case.oh, case.ow, _lib.ptr(xo), _lib.ptr(xa),
                                              _lib.ptr(yo), _lib.ptr(ya), stream()), "demia_resize_linear_u8")
    torch.cuda.synchronize()
    assert guards_intact(whole, CANARY8)
    got = dst.view(want.shape)
    assert torch.equal(got, want), describe_difference(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# 3. stem, pools, subsample
# ---------------------------------------------------------------------------------------------------------------------
def stem_state(env, case):
    """Per case, built once: the operands on the device (the input between NaNs), the f64 references, the plane scales."""
    key = ("stem", case)
    if key not in env.cache:
        from deepemia_amd import engine as E
        from deepemia_amd import p32
        dev = env.dev
        ops = S.stem_operands(case)
        x = R.stem_input(ops["bytes"])
        dh, dw = case.ph + 6, case.pw + 8
        tail = 40 * dw * 4                                        # more than the 37 rows a workgroup stages
        around = torch.full((GUARD + x.numel() + tail,), float("nan"), dtype=torch.float32, device=dev)
        around[GUARD:GUARD + x.numel()] = x.reshape(-1).to(dev)
        ws = torch.zeros((7, 8, 4, 64), dtype=torch.float32)
        ws[:, :7, :3, :] = ops["wt"].permute(2, 3, 1, 0)
        planes, sw = E.stem_weight_planes(ops["wt"])
        s_in = p32.plane_scale(255.0 - min(S.PIXEL_MEAN))
        ref = R.stem_reference(ops)
        env.cache[key] = SimpleNamespace(
            ops=ops, around=around, xin=around[GUARD:GUARD + x.numel()], image_bytes=dh * dw * 16, w=ws.to(dev), planes=planes.to(dev).contiguous(),
            scale=ops["scale"].to(dev), scale_mfma=(ops["scale"] / (sw * s_in)).to(dev).contiguous(), bias=ops["bias"].to(dev), s_in=s_in,
            s_out=p32.plane_scale(S.stem_bound(ops)), ref=ref.to(dev), pooled=R.pool_reference(ref).to(dev))
    return env.cache[key]


def stem_launch(env, st, case, which, image=None):
    """``demia_stem_conv`` (f32) or ``demia_stem_conv_mfma`` on the whole batch, or on image ``image`` alone.  Returns (whole, [n, Ho, Wo, 64] f32)."""
    from deepemia_amd import _lib
    n = case.n if image is None else 1
    src = _lib.ptr(st.xin) + (0 if image is None else image * st.image_bytes)
    ho, wo = case.ph // 2, case.pw // 2
    whole, mid = guarded(env.dev, n * ho * wo * 64, torch.int32, CANARY32)
    if which == "f32":
        _lib.check(env.lib.demia_stem_conv(src, _lib.ptr(st.w), _lib.ptr(st.scale), _lib.ptr(st.bias), _lib.ptr(mid), n, case.ph, case.pw, _lib.F32,
                                           stream()), "demia_stem_conv")
    else:
        _lib.check(env.lib.demia_stem_conv_mfma(src, _lib.ptr(st.planes), _lib.ptr(st.scale_mfma), _lib.ptr(st.bias), _lib.ptr(mid), n, case.ph,
                                                case.pw, st.s_in, stream()), "demia_stem_conv_mfma")
    torch.cuda.synchronize()
    return whole, mid.view(torch.float32).view(n, ho, wo, 64)


def normalised_error(got, ref) -> float:
    return float((got.double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("which", ["f32", "mfma"])
@pytest.mark.parametrize("case", S.STEM_CASES, ids=lambda c: c.name)
def test_stem_conv_against_f64(env, case, which):
    st = stem_state(env, case)
    whole, got = stem_launch(env, st, case, which)
    assert guards_intact(whole, CANARY32)
    err = normalised_error(got, st.ref)
    print(f"stem {which} {case.name}: err = {err:.3e} of max |y| = {float(st.ref.abs().max()):.6e}")
    assert err <= S.BAR, err
    assert not bool(got[..., S.ZERO_CHANNEL].ne(0.25).any())            # the all-zero channel is its bias, exactly
    if case.n > 1:                                                       # an image alone = the same image inside the batch
        for i in (1, case.n - 1):
            w1, one = stem_launch(env, st, case, which, image=i)
            assert guards_intact(w1, CANARY32)
            assert torch.equal(one[0], got[i]), (i, describe_difference(one[0], got[i]))


def p32_buffer(dev, pixels, channels):
    """(whole, body) as int16: a zero header of 128 bytes, then the planes, canaries all around."""
    whole, body = guarded(dev, 64 + 2 * pixels * channels, torch.int16, CANARY16)
    body[:64] = 0
    return whole, body


def meta_buffer(dev, groups):
    whole, body = guarded(dev, 2 * groups, torch.int32, CANARY32)
    body.zero_()
    return whole, body


@pytest.mark.parametrize("case", S.STEM_CASES, ids=lambda c: c.name)
def test_stem_pool_fused_equals_the_two_kernels_and_f64(env, case):
    from deepemia_amd import _lib
    st = stem_state(env, case)
    lib, dev = env.lib, env.dev
    ho, wo, hp, wp = case.ph // 2, case.pw // 2, case.ph // 4, case.pw // 4
    pixels = case.n * hp * wp
    _, mid = stem_launch(env, st, case, "mfma")
    amax = float(st.pooled.abs().max())
    high = {}
    for groups in sorted({1, case.n}):
        for single in (0, 1):
            fw, fused = p32_buffer(dev, pixels, 64)
            fmw, fmeta = meta_buffer(dev, groups)
            _lib.check(lib.demia_stem_pool_mfma(_lib.ptr(st.xin), _lib.ptr(st.planes), _lib.ptr(st.scale_mfma), _lib.ptr(st.bias), _lib.ptr(fused),
                                                _lib.ptr(fmeta), case.n, case.ph, case.pw, st.s_in, st.s_out, groups, single, stream()),
                       "demia_stem_pool_mfma")
            tw, two = p32_buffer(dev, pixels, 64)
            tmw, tmeta = meta_buffer(dev, groups)
            _lib.check(lib.demia_maxpool3x3s2_p32(_lib.ptr(mid), _lib.ptr(two), _lib.ptr(tmeta), st.s_out, case.n, ho, wo, 64, groups, single,
                                                  stream()), "demia_maxpool3x3s2_p32")
            torch.cuda.synchronize()
            what = f"groups = {groups}, single = {single}"
            for whole, canary in ((fw, CANARY16), (tw, CANARY16), (fmw, CANARY32), (tmw, CANARY32)):
                assert guards_intact(whole, canary), what
            assert not bool(fused[:64].any()) and not bool(two[:64].any()), what          # the 128-byte header is still zero
            assert torch.equal(fused, two), (what, describe_difference(fused, two))
            assert torch.equal(fmeta, tmeta), (what, fmeta.view(torch.float32).tolist(), tmeta.view(torch.float32).tolist())
            meta = fmeta.view(torch.float32).view(groups, 2)
            assert bool((meta[:, 1] == st.s_out).all()), what
            want_max = st.pooled.reshape(groups, -1).amax(dim=1)
            assert bool(((meta[:, 0].double() - want_max).abs() <= S.BAR * amax).all()), (what, meta[:, 0].tolist(), want_max.tolist())
            assert float(meta[:, 0].max()) * st.s_out < 32768.0
            planes = fused[64:].view(torch.float16).view(pixels, 2, 2, 32)
            if single:
                assert not bool(planes[:, :, 1].any()), what
                assert torch.equal(planes[:, :, 0], high[groups]), what
            else:
                high[groups] = planes[:, :, 0].clone()
                got = ((planes[:, :, 0].double() + planes[:, :, 1].double()) / st.s_out).reshape(case.n, hp, wp, 64)
                err = normalised_error(got, st.pooled)
                print(f"stem + pool {case.name}, {what}: err = {err:.3e} of max |y| = {amax:.6e}")
                assert err <= S.BAR, (what, err)
    assert torch.equal(high[1], high[case.n])                     # the planes do not depend on the grouping (one host-side scale)


@pytest.mark.parametrize("case", S.POOL_P32_CASES, ids=lambda c: c.name)
def test_maxpool_p32_equals_the_plane_split_restated(env, case):
    from deepemia_amd import _lib, p32
    x = S.pool_input(case)
    s = p32.plane_scale(float(x.abs().max()))
    pooled = R.pool_reference(x)                                  # f32: a maximum is exact
    ho, wo = S.pooled_extent(case.h), S.pooled_extent(case.w)
    xd = x.to(env.dev)
    for groups in sorted({1, case.n}):
        for single in (0, 1):
            whole, out = p32_buffer(env.dev, case.n * ho * wo, case.c)
            mw, meta = meta_buffer(env.dev, groups)
            _lib.check(env.lib.demia_maxpool3x3s2_p32(_lib.ptr(xd), _lib.ptr(out), _lib.ptr(meta), s, case.n, case.h, case.w, case.c, groups, single,
                                                      stream()), "demia_maxpool3x3s2_p32")
            torch.cuda.synchronize()
            what = f"groups = {groups}, single = {single}"
            assert guards_intact(whole, CANARY16) and guards_intact(mw, CANARY32), what
            assert not bool(out[:64].any()), what
            planes, want_meta = R.p32_planes(pooled, s, groups, bool(single))
            got = out[64:].cpu()
            assert torch.equal(got, planes.view(torch.int16).reshape(-1)), (what, describe_difference(got, planes.view(torch.int16).reshape(-1)))
            assert torch.equal(meta.view(torch.float32).view(groups, 2).cpu(), want_meta), (what, meta.view(torch.float32).tolist(), want_meta.tolist())
            if single:
                assert not bool(out[64:].view(-1, 2, 32)[:, 1].any())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", S.POOL_CASES, ids=lambda c: c.name)
def test_maxpool_and_subsample2_are_exact(env, case, dtype):
    from deepemia_amd import _lib
    code = _lib.F32 if dtype == torch.float32 else _lib.BF16
    bits, canary = (torch.int32, CANARY32) if dtype == torch.float32 else (torch.int16, CANARY16)
    x = S.pool_input(case).to(dtype)
    xd = x.to(env.dev)
    want = R.pool_reference(x.float()).to(dtype)
    whole, out = guarded(env.dev, want.numel(), bits, canary)
    _lib.check(env.lib.demia_maxpool3x3s2(_lib.ptr(xd), _lib.ptr(out), case.n, case.h, case.w, case.c, code, stream()), "demia_maxpool3x3s2")
    torch.cuda.synchronize()
    assert guards_intact(whole, canary)
    got = out.view(dtype).view(want.shape).cpu()
    assert torch.equal(got.view(bits), want.view(bits)), describe_difference(got, want)
    want = x[:, ::2, ::2].contiguous()
    whole, out = guarded(env.dev, want.numel(), bits, canary)
    _lib.check(env.lib.demia_subsample2(_lib.ptr(xd), _lib.ptr(out), case.n, case.h, case.w, case.c, code, stream()), "demia_subsample2")
    torch.cuda.synchronize()
    assert guards_intact(whole, canary)
    got = out.view(dtype).view(want.shape).cpu()
    assert torch.equal(got.view(bits), want.view(bits)), describe_difference(got, want)


def test_subsample2_of_p32_pixels_behind_their_header(env):
    """P6 as the f16x2 engine makes it: a P32 pixel of 256 channels is 256 four-byte words, the copy runs as F32 on pointers moved
    past the 128-byte headers (``_lib.ptr(t) + 128``).  Headers and canaries stay, every pixel is the right one."""
    from deepemia_amd import _lib
    n, h, w, c = 2, 25, 42, 256
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    g = torch.Generator().manual_seed(9)
    sw, src = p32_buffer(env.dev, n * h * w, c)
    src[64:] = torch.randint(-32768, 32768, (2 * n * h * w * c,), generator=g, dtype=torch.int16).to(env.dev)
    dw, dst = p32_buffer(env.dev, n * ho * wo, c)
    _lib.check(env.lib.demia_subsample2(_lib.ptr(src) + 128, _lib.ptr(dst) + 128, n, h, w, c, _lib.F32, stream()), "demia_subsample2")
    torch.cuda.synchronize()
    assert guards_intact(dw, CANARY16) and guards_intact(sw, CANARY16)
    assert not bool(dst[:64].any())
    want = src[64:].view(n, h, w, 2 * c)[:, ::2, ::2].contiguous()
    assert torch.equal(dst[64:].view(n, ho, wo, 2 * c), want)
