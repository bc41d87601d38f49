"""Every product tile of ``conv_p32_kernel`` against float64 references, and against each other bit for bit.

``demia_conv2d_p32`` dispatches to nine tile shapes with the straight-line planes epilogue (``kTiles``: 1 = 256 x 256,
2 = 128 x 256, 4 = 192 x 256, 12 = 160 x 256, 13 = 224 x 256, 6 = 256 x 128, 7 = 128 x 128, 9 = 256 x 64, 11 = 128 x 64) and
to four with the guarded epilogue (f32 outputs, ``Cout % 64 == 32``: 7G, 9G, 10G, 11G); ``single != 0`` goes to a second
compile of the same file.  Each is its own template instantiation -- wave grid, epilogue passes, the rows a ragged last
tile owns, the scale groups a tile can straddle -- and a cost model picks one per launch, so which one a layer runs changes
with the batch size.  The older kernel-level tests never pass a hint; the restated model (``conv_p32_cases.resolve``, checked
in ``test_cpu_conv_p32_tile_list.py``) says what they reach:

  ``CONV_CASES`` of test_gpu_parity_nn.py, in order: 11, 11, 11, 11, 11, 11G, 11, 11, 4, 11, 1
  ``test_conv_p32_scale_groups_equal_the_images_alone``: 11, 11, 11G, 11
  ``test_single_plane_conv_is_the_high_plane_product``: no hint either; the fused-head tests hint 1, 2 and 4 (another epilogue)

Here every tile is forced by ``tile_hint``:

1. ``test_tile_against_f64``: tile x case sweep (``conv_p32_cases.CASES``: single K-step, odd K-step count with RES_SAME,
   stride 2 on odd sizes, 3 x 3 over three images, RES_UP2 on odd sizes, 72 K-steps, the fully-connected shape, more than
   520 workgroups), rows chosen per tile (one partial tile, whole tiles exactly, ragged remainders, a workgroup count on
   every residue mod 8), through the C ABI into a caller-owned buffer: 128-byte header, M rows, 256 rows of a canary
   pattern.  Bar 2e-5 of max |reference|, ``meta`` checked, header still zero, canary untouched -- the straight-line
   epilogue relies on the hardware bound ``out_bytes`` to drop the rows >= M of a ragged tile.  For f32 outputs the padding
   columns ``Cout .. out_ld`` are LEFT ALONE (the guarded epilogue stores ``co < Cout`` only); the test holds the kernel
   to that.  Tile 10G is reachable by hint only (not in ``kTiles``, not the fall-back of any hint): dead in the product,
   swept all the same.  7G refuses ``CoutPad % 128 != 0``: DEMIA_EINVAL, output untouched, then skipped.
   A hinted 256- or 128-wide tile whose width does not divide Cout is not refused: it falls back to 7G / 11G.
2. ``test_tiles_agree_bit_for_bit``: for every case, planes and meta are ``torch.equal`` among the straight-line tiles and,
   separately, among the guarded tiles.  The epilogue kind depends on Cout and ``out_f32`` only, never on M, so identity
   within a kind is what batch invariance needs; across kinds nothing is required (the two epilogues round the scale /
   bias / residual chain differently: packed f32 multiplies and fused residual FMAs against plain ones).
   The outcome is recorded at the end of this docstring.
3. ``test_scale_groups_*``: five images 100x apart in amplitude in one launch, 128 and 144 rows per image, no residual /
   RES_SAME / RES_UP2, on every tile: each image equals bit for bit what the same tile gives it alone; a grouped tensor
   sent in two calls with ``row0`` equals the single call; rows outside ``groups`` are refused.
4. ``test_single_plane_*``: the single-plane compile under every hint it accepts, against the f64 product of the high
   planes (3e-6), K-step of 64 (Cin % 64 == 0) and of 32 (Cin = 96), ``single = 2``, bit identity across tiles.

References are float64 torch on the CPU, computed once per case at the largest row count and sliced per tile.

OUTCOME of 2, measured on an MI355X: IDENTICAL.  All nine straight-line tiles agree bit for bit (planes and meta) on every
case, so do the four guarded tiles, in the two-plane and in the single-plane compile, with the product and with the dev
library.  Largest error against f64 over the sweep: 1.1e-6 of max |reference| (bar 2e-5).  Wall time of the module: 3 s
(24 s in a first run on a cold machine) with either library, 352 passed and 5 skipped (7G at CoutPad = 64);
test_gpu_parity_nn.py took 20 s in the same run.
"""
import ctypes as C
import math
from types import SimpleNamespace

import pytest
import torch

import conv_p32_cases as S

pytestmark = pytest.mark.gpu

CANARY16 = 0x7BCD            # fp16 bit pattern of the rows behind the tensor
CANARY32 = 0x7FC0BEEF        # f32 bit pattern (a NaN payload) of an f32 output buffer before the launch
DEMIA_EINVAL = -1


@pytest.fixture(scope="module")
def env(gpu_device):
    """Per case, built on first use and kept: the layer, the operands as P32 on the device and the f64 reference.  The
    engine (for ``conv_p32``) never runs a forward, so every output is a fresh allocation."""
    from deepemia_amd import _lib
    state = dict(engine=None)

    def engine():
        if state["engine"] is None:
            from deepemia_amd import synth
            from deepemia_amd.engine import MaskRCNNEngine
            state["engine"] = MaskRCNNEngine(synth.random_d2_state_dict(50, 2, seed=0), 50, 2, 0.3, gpu_device, "f16x2")
        return state["engine"]

    yield SimpleNamespace(dev=gpu_device, lib=_lib.load(), cache={}, engine=engine)
    state.clear()


def make_layer(dev, wt, scale, bias, stride, pad, cout_pad=None, single=0):
    """As test_single_plane_conv_is_the_high_plane_product builds it.  Returns (ConvLayer, fp16 planes, per-channel weight scale)."""
    from deepemia_amd import engine as E
    cout, cin, k, _ = wt.shape
    cout_pad = cout_pad or S.cdiv(cout, 64) * 64
    wp = torch.zeros((cout_pad, k, k, cin))
    wp[:cout] = wt.permute(0, 2, 3, 1)
    planes, sw = E.split2_f16_scaled(wp.to(dev))
    L = E.ConvLayer(None, scale.to(dev), bias.to(dev), cin, cout, cout_pad, k, k, stride, pad, E.tile_weight_planes_p32(planes),
                    (scale.to(dev) / sw[:cout]).contiguous(), float((scale.abs() * wt.abs().flatten(1).sum(1)).max()), float(bias.abs().max()),
                    single=single)
    return L, planes, sw


def case_state(env, case, n=None, single=0):
    key = (case.name, n, single)
    if key not in env.cache:
        from deepemia_amd import p32
        ops = S.operands(case, n)
        L, planes, sw = make_layer(env.dev, ops["wt"], ops["scale"], ops["bias"], case.stride, case.pad, single=single)
        xp = p32.from_f32(ops["x"].to(env.dev))
        rp = None if ops["res"] is None else p32.from_f32(ops["res"].to(env.dev))
        env.cache[key] = SimpleNamespace(ops=ops, L=L, planes=planes, sw=sw, xp=xp, rp=rp, ref=None)
    return env.cache[key]


def reference_on_device(env, case, st):
    if st.ref is None:
        st.ref = S.reference(case, st.ops).to(env.dev)
    return st.ref


def out_buffer(dev, m, cout, out_f32, ld):
    """Caller-owned output: planes = 128 zero bytes, then (m + 256) rows of the canary; f32 = (m + 256) rows of ``ld`` canaries."""
    if out_f32:
        return torch.full(((m + 256) * ld,), CANARY32, dtype=torch.int32, device=dev)
    buf = torch.full((64 + (m + 256) * cout * 2,), CANARY16, dtype=torch.int16, device=dev)
    buf[:64] = 0
    return buf


def call(env, L, x_ptr, x_meta, n, h, w, out, meta, tile, act, res_ptr=0, res_meta=0, res_mode=0, out_f32=False, out_ld=0,
         groups=1, group_rows=0, row0=0, single=0, out_ofs=0):
    from deepemia_amd import _lib
    ho = (h + 2 * L.pad - L.kh) // L.stride + 1
    wo = (w + 2 * L.pad - L.kw) // L.stride + 1
    d = _lib.ConvP32Desc(x_ptr, x_meta, _lib.ptr(L.w3), _lib.ptr(L.scale3), _lib.ptr(L.bias), res_ptr, res_meta, _lib.ptr(out) + out_ofs,
                         0 if out_f32 else _lib.ptr(meta), L.wbound, L.bbound, n, h, w, L.cin, ho, wo, L.cout, L.cout_pad, L.kh, L.kw,
                         L.stride, L.pad, act, res_mode, 1 if out_f32 else 0, out_ld, tile, 0, 0, 0, 0, 0, 0,
                         groups, group_rows if groups > 1 else n * ho * wo, row0, single)
    status = env.lib.demia_conv2d_p32(C.byref(d), int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return status


def launch_case(env, tile, case, st, n):
    """One launch of the first ``n`` images of the case's operands under ``tile``.  Returns (status, raw buffer, meta, M)."""
    from deepemia_amd import _lib
    m = n * case.ho * case.wo
    out = out_buffer(env.dev, m, case.cout, case.out_f32, case.ld)
    meta = torch.zeros((1, 2), dtype=torch.float32, device=env.dev)
    status = call(env, st.L, _lib.ptr(st.xp.buf), _lib.ptr(st.xp.meta), n, case.h, case.w, out, meta, tile.id, 1 if case.relu else 0,
                  0 if st.rp is None else _lib.ptr(st.rp.buf), 0 if st.rp is None else _lib.ptr(st.rp.meta), case.res,
                  case.out_f32, case.out_ld)
    return status, out, meta, m


def untouched(out, meta, case, m):
    fresh = out_buffer(out.device, m, case.cout, case.out_f32, case.ld)
    return torch.equal(out, fresh) and not bool(meta.any())


def rows_of(out, meta, case, m):
    """The tensor the launch wrote, as f32 [M, Cout]."""
    from deepemia_amd import p32
    if case.out_f32:
        return out.view(torch.float32).view(m + 256, case.ld)[:m, :case.cout]
    return p32.to_f32(p32.P32(out.view(torch.float16)[:64 + 2 * m * case.cout], meta, (m, case.cout)))


# ------------------------------------------------------------------------------------------------------------------
# 1. tile x case against f64
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile,case", S.SWEEP, ids=[f"t{t.name}-{c.name}" for t, c in S.SWEEP])
def test_tile_against_f64(env, tile, case):
    st = case_state(env, case)
    n = S.rows_for(tile, case)
    status, out, meta, m = launch_case(env, tile, case, st, n)
    if S.refused(tile, case):
        assert status == DEMIA_EINVAL, status
        assert untouched(out, meta, case, m)
        pytest.skip(f"tile {tile.name} refuses CoutPad = {case.cout_pad} by contract (DEMIA_EINVAL, output untouched)")
    assert status == 0, env.lib.demia_last_error()
    ref = reference_on_device(env, case, st)[:m]
    got = rows_of(out, meta, case, m)
    amax_ref = float(ref.abs().max())
    err = S.normalised_error(got, ref)
    print(f"tile {tile.name} {case.name}: M = {m}, nwg = {S.nwg(tile, case, n)}, err = {err:.3e}, max |y| = {amax_ref:.6e}, meta = {meta.tolist()}")
    assert err <= S.BAR, err
    if case.out_f32:
        raw = out.view(m + 256, case.ld)
        assert bool((raw[:m, case.cout:] == CANARY32).all()), "padding columns Cout .. out_ld were written"
        assert bool((raw[m:] == CANARY32).all()), "rows >= M were written"
        assert not bool(meta.any())
    else:
        assert not bool(out[:64].any()), "the zero header was written"
        assert bool((out[64 + 2 * m * case.cout:] == CANARY16).all()), "rows >= M were written"
        amax, s = float(meta[0, 0]), float(meta[0, 1])
        assert abs(amax - amax_ref) <= 1e-5 * amax_ref, (amax, amax_ref)
        assert s > 0 and math.frexp(s)[0] == 0.5, s          # an exact power of two
        assert amax * s < 32768.0, (amax, s)


def test_hints_refused_by_contract_leave_the_output_untouched(env):
    """``CoutPad % 256`` / ``CoutPad % 128``: a hinted tile wider than the padded channel count divides is DEMIA_EINVAL before
    anything is launched.  (Natural padding, CoutPad = roundup(Cout, 64), only ever meets this on 7G: the sweep's skips.)"""
    g = torch.Generator().manual_seed(77)
    combos = [(t, 256, 320, False) for t in (1, 2, 4, 12, 13)] + [(6, 128, 192, False), (7, 128, 192, False), (7, 80, 192, True), (7, 15, 64, True)]
    from deepemia_amd import _lib, p32
    x = p32.from_f32(torch.randn((300, 1, 1, 64), generator=g).to(env.dev))
    for tile, cout, cout_pad, out_f32 in combos:
        L, _, _ = make_layer(env.dev, torch.randn((cout, 64, 1, 1), generator=g) / 8, torch.rand((cout,), generator=g) + 0.5,
                             torch.randn((cout,), generator=g), 1, 0, cout_pad=cout_pad)
        case = SimpleNamespace(cout=cout, out_f32=out_f32, ld=cout)
        out = out_buffer(env.dev, 300, cout, out_f32, cout)
        meta = torch.zeros((1, 2), dtype=torch.float32, device=env.dev)
        status = call(env, L, _lib.ptr(x.buf), _lib.ptr(x.meta), 300, 1, 1, out, meta, tile, 1, out_f32=out_f32)
        assert status == DEMIA_EINVAL, (tile, cout, cout_pad, status)
        assert b"CoutPad" in env.lib.demia_last_error()
        assert untouched(out, meta, case, 300), (tile, cout, cout_pad)


# ------------------------------------------------------------------------------------------------------------------
# 2. tile independence
# ------------------------------------------------------------------------------------------------------------------
def describe_difference(a, b):
    d = (a != b).nonzero().flatten()
    return f"{d.numel()} of {a.numel()} elements differ, first at {d[:4].tolist()}" if a.shape == b.shape else f"shapes {a.shape} / {b.shape}"


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_tiles_agree_bit_for_bit(env, case):
    st = case_state(env, case)
    n = S.n_common(case)
    tiles = [t for t in S.TILES if S.runs_on(t, case) and not S.refused(t, case)]
    assert len(tiles) >= 2
    first = None
    for t in tiles:
        status, out, meta, m = launch_case(env, t, case, st, n)
        assert status == 0, (t.name, env.lib.demia_last_error())
        if first is None:
            first = (t, out, meta)
            assert case.out_f32 or float(meta[0, 0]) > 0
            continue
        assert torch.equal(out, first[1]), (t.name, first[0].name, describe_difference(out, first[1]))
        assert torch.equal(meta, first[2]), (t.name, first[0].name, meta.tolist(), first[2].tolist())


# ------------------------------------------------------------------------------------------------------------------
# 3. scale groups on every tile
# ------------------------------------------------------------------------------------------------------------------
def group_layer(env, tile, k, pad):
    cout = 96 if tile.guarded else 256
    key = ("group", cout, k)
    if key not in env.cache:
        g = torch.Generator().manual_seed(300 + cout + k)
        wt = torch.randn((cout, 64, k, k), generator=g) / (64 * k * k) ** 0.5
        env.cache[key] = make_layer(env.dev, wt, torch.rand((cout,), generator=g) + 0.5, torch.randn((cout,), generator=g) * 0.1, 1, pad)[0]
    return env.cache[key]


@pytest.mark.parametrize("res", [S.RES_NONE, S.RES_SAME, S.RES_UP2], ids=["nores", "same", "up2"])
@pytest.mark.parametrize("geo", S.GROUP_GEOS, ids=lambda g: g[0])
@pytest.mark.parametrize("tile", S.TILES, ids=lambda t: f"t{t.name}")
def test_scale_groups_equal_the_images_alone_on_every_tile(env, tile, geo, res):
    """test_conv_p32_scale_groups_equal_the_images_alone under every tile hint: 128 rows per image (group boundaries on tile
    boundaries, the documented minimum) and 144 (a 256-row tile meets three groups)."""
    from deepemia_amd import p32
    from deepemia_amd._lib import ACT_RELU

    _, h, w, k, pad = geo
    eng, dev, n = env.engine(), env.dev, len(S.GROUP_AMPS)
    L = group_layer(env, tile, k, pad)
    g = torch.Generator().manual_seed(h * 100 + k * 10 + res)
    amp = torch.tensor(S.GROUP_AMPS).view(n, 1, 1, 1)
    x = torch.randn((n, h, w, 64), generator=g) * amp
    r = None
    if res == S.RES_SAME:
        r = torch.randn((n, h, w, L.cout), generator=g) * amp
    elif res == S.RES_UP2:
        r = torch.randn((n, (h + 1) // 2, (w + 1) // 2, L.cout), generator=g) * amp
    xp = p32.from_f32(x.to(dev), groups=n)
    rp = None if r is None else p32.from_f32(r.to(dev), groups=n)
    assert len(set(xp.meta[:, 1].tolist())) > 1
    out = eng.conv_p32(xp, L, act=ACT_RELU, residual=rp, res_mode=res, tile_hint=tile.id)
    torch.cuda.synchronize()
    assert out.groups == n and float(out.meta[:, 0].min()) > 0
    per = h * w * L.cout * 2
    for i in range(n):
        xi = p32.from_f32(x[i:i + 1].to(dev))
        ri = None if r is None else p32.from_f32(r[i:i + 1].to(dev))
        oi = eng.conv_p32(xi, L, act=ACT_RELU, residual=ri, res_mode=res, tile_hint=tile.id)
        torch.cuda.synchronize()
        assert torch.equal(oi.meta[0], out.meta[i]), (i, oi.meta.tolist(), out.meta.tolist())
        assert torch.equal(oi.buf[64:], out.buf[64 + i * per:64 + (i + 1) * per]), i


@pytest.mark.parametrize("c0", [256, 300])
@pytest.mark.parametrize("tile", S.TILES, ids=lambda t: f"t{t.name}")
def test_scale_groups_in_two_calls_with_row0_equal_the_single_call(env, tile, c0):
    """A grouped H = W = 1 tensor (five groups of 128 rows) in two calls, the second with ``row0 = c0`` and all pointers moved
    on by c0 rows, as the more-than-4-GiB chunking of ``engine.conv_p32`` does (which cuts at multiples of 256; 300 cuts
    inside a group and inside a row pair): planes and ``out_meta`` equal the single call's bit for bit.  Rows that fall
    outside ``groups`` are refused."""
    from deepemia_amd import _lib, p32

    dev, groups, rows = env.dev, 5, 128
    m = groups * rows
    L = group_layer(env, tile, 1, 0)
    g = torch.Generator().manual_seed(4000 + c0)
    amp = torch.tensor(S.GROUP_AMPS).repeat_interleave(rows).view(m, 1, 1, 1)
    xp = p32.from_f32((torch.randn((m, 1, 1, 64), generator=g) * amp).to(dev), groups=groups)
    rp = p32.from_f32((torch.randn((m, 1, 1, L.cout), generator=g) * amp).to(dev), groups=groups)
    case = SimpleNamespace(cout=L.cout, out_f32=False, ld=L.cout)

    def run(pieces, row0_of=lambda c: c):
        out = out_buffer(dev, m, L.cout, False, L.cout)
        meta = torch.zeros((groups, 2), dtype=torch.float32, device=dev)
        status = []
        for c, cn in pieces:
            status.append(call(env, L, _lib.ptr(xp.buf) + c * 64 * 4, _lib.ptr(xp.meta), cn, 1, 1, out, meta, tile.id, 1,
                               _lib.ptr(rp.buf) + c * L.cout * 4, _lib.ptr(rp.meta), S.RES_SAME, groups=groups, group_rows=rows,
                               row0=row0_of(c), out_ofs=c * L.cout * 4))
        return status, out, meta

    s1, whole, meta1 = run([(0, m)])
    s2, parts, meta2 = run([(0, c0), (c0, m - c0)])
    assert s1 == [0] and s2 == [0, 0], (s1, s2, env.lib.demia_last_error())
    assert float(meta1.min()) > 0
    assert torch.equal(parts, whole), describe_difference(parts, whole)
    assert torch.equal(meta2, meta1), (meta2.tolist(), meta1.tolist())
    assert not bool(whole[:64].any()) and bool((whole[64 + 2 * m * L.cout:] == CANARY16).all())
    s3, out3, meta3 = run([(0, m)], row0_of=lambda c: 1)          # (M + row0) reaches into a sixth group
    assert s3 == [DEMIA_EINVAL] and untouched(out3, meta3, case, m)


# ------------------------------------------------------------------------------------------------------------------
# 4. the single-plane compile
# ------------------------------------------------------------------------------------------------------------------
SINGLE_GEOS = {"k3c256": ("k3c256-o256", "k3c256-o96", 3), "k1c64": ("many-o256", "many-o96", 3001), "k1c96same": ("k1c96same-o512", "k1c96same-o96", 1003)}


def single_case(tile, geo):
    plain, guarded, n = SINGLE_GEOS[geo]
    name = guarded if tile.guarded else plain
    return next(c for c in S.CASES if c.name == name), n


def run_single(env, tile, case, n, single):
    st = case_state(env, case, n, single)
    out = env.engine().conv_p32(st.xp, st.L, act=1 if case.relu else 0, residual=st.rp, res_mode=case.res, tile_hint=tile.id)
    torch.cuda.synchronize()
    return st, out


@pytest.mark.parametrize("geo", list(SINGLE_GEOS))
@pytest.mark.parametrize("tile", S.TILES, ids=lambda t: f"t{t.name}")
def test_single_plane_compile_on_every_tile(env, tile, geo):
    """``single = 1`` under every hint: ONE MFMA per product on the high planes of both operands.  Reference and bar of
    test_single_plane_conv_is_the_high_plane_product -- the f64 convolution of exactly those planes (the residual enters
    with both planes), 3e-6 of max |out| -- and the results of all tiles of a kind are bit-identical."""
    from deepemia_amd import p32

    case, n = single_case(tile, geo)
    st, out = run_single(env, tile, case, n, 1)
    if st.ref is None:
        xh = st.xp.buf[p32.HEADER_HALFS:].view(-1, case.cin // 32, 2, 32)[:, :, 0, :].reshape(n, case.h, case.w, case.cin).double() / float(st.xp.meta[0, 1])
        wh = (st.planes[0].double() / st.sw.double().view(-1, 1, 1, 1))[:case.cout].permute(0, 3, 1, 2)
        ops = dict(st.ops, x=xh.cpu(), wt=wh.cpu(), res=None if st.rp is None else p32.to_f32(st.rp).double().cpu())
        st.ref = S.reference(case, ops).to(env.dev)
        st.first = (tile, out)
    got = p32.to_f32(out).reshape(-1, case.cout)
    err = S.normalised_error(got, st.ref)
    print(f"single, tile {tile.name} {case.name}: err = {err:.3e}")
    assert err < S.SINGLE_BAR, err
    amax = float(st.ref.abs().max())
    assert abs(float(out.meta[0, 0]) - amax) <= 1e-5 * amax
    assert torch.equal(out.buf, st.first[1].buf), (tile.name, st.first[0].name, describe_difference(out.buf, st.first[1].buf))
    assert torch.equal(out.meta, st.first[1].meta)


@pytest.mark.parametrize("tile", S.TILES, ids=lambda t: f"t{t.name}")
def test_single_plane_zero_low_output(env, tile):
    """``single = 2``: the low plane is all zeros and the high plane (and meta) is the one ``single = 1`` writes."""
    case, n = single_case(tile, "k3c256")
    _, one = run_single(env, tile, case, n, 1)
    _, two = run_single(env, tile, case, n, 2)
    a = one.buf[64:].view(-1, case.cout // 32, 2, 32)
    b = two.buf[64:].view(-1, case.cout // 32, 2, 32)
    assert torch.equal(b[:, :, 0], a[:, :, 0]) and bool(a[:, :, 1].any())
    assert not bool(b[:, :, 1].any())
    assert torch.equal(one.meta, two.meta)
