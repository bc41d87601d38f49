"""The RPN predictor fused into the RPN conv's epilogue (``demia_conv_p32_desc.head_planes``) against the two launches it replaces.

The contract of the fused launch is BIT IDENTITY: a planes layer (3 x 3, 256 -> 256, ReLU) whose epilogue hands its two fp16
planes to a 1 x 1 f32-out layer of at most 16 channels through LDS must give exactly what the planes layer followed by the
stand-alone 1 x 1 launch gives -- the same per-image output scale, the same split of ``v * s`` into high and low plane, the same
product order (channel groups 0..7, ``a_h b_l``, ``a_l b_h``, ``a_h b_h`` per group).

1. ``test_fused_equals_two_launches``: through the C ABI into caller-owned buffers, every fused tile shape (hints 1 = 256 x 256,
   2 = 128 x 256, 4 = 192 x 256, 15 = 64 x 256: the small-M tile of this mode) x three geometries x Cout in {15, 1, 16}:
     3 images of 13 x 13 (M = 507: a 256-row tile meets three images, the last tile has rows >= M),
     2 images of 25 x 25 (an image boundary inside a tile), 1 image of 50 x 50 (several tiles, M % 256 != 0).
   Per-image magnitudes differ by non-power-of-two factors of at least 2^6 (the three per-image scale selects differ), one image
   of the three is all zeros (its bound reduces to ``bbound``), predictor rows are negative / near zero.  ``torch.equal`` on the
   [M, Cout] heads; rows >= M and columns >= Cout of the fused launch's buffer keep their canary (the two-launch path leaves
   them alone as well).
2. ``test_fused_against_f64``: the fused heads against the float64 reference of ``conv_p32_cases`` (conv, ReLU, 1 x 1) at that
   module's bar, so that the module does not lean on its sibling launch only.
3. ``test_fused_launch_refuses_what_it_cannot_do``: preconditions of the mode are DEMIA_EINVAL, nothing written.
4. ``test_engine_rpn_fused_equals_two_launches``: R50 on one 256 x 256 image: ``rpn_fused`` on and off give identical heads,
   proposals, scores and counts; eager forward and graph replay agree.
"""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import conv_p32_cases as S

pytestmark = pytest.mark.gpu

CANARY32 = 0x7FC0BEEF
DEMIA_EINVAL = -1
ACT_RELU = 1
LD = 16

GEOS = {"3x13x13": (3, 13, 13, (1.0, 0.0, 83.0)), "2x25x25": (2, 25, 25, (0.37, 0.37 * 75.0)), "1x50x50": (1, 50, 50, (5.3,))}
FUSED_TILES = (1, 2, 4, 15)
COUTS = (15, 1, 16)


def make_layer(dev, wt, bias, pad):
    """A bias-only layer as ``MaskRCNNEngine._conv`` packs it (no FrozenBN scale)."""
    from deepemia_amd import engine as E
    cout, cin, k, _ = wt.shape
    cout_pad = S.cdiv(cout, 64) * 64
    wp = torch.zeros((cout_pad, k, k, cin))
    wp[:cout] = wt.permute(0, 2, 3, 1)
    planes, sw = E.split2_f16_scaled(wp.to(dev))
    return E.ConvLayer(None, None, bias.to(dev).contiguous(), cin, cout, cout_pad, k, k, 1, pad, E.tile_weight_planes_p32(planes),
                       (1.0 / sw[:cout]).contiguous(), float(wt.abs().flatten(1).sum(1).max()), float(bias.abs().max()))


def predictor_weights(cout):
    g = torch.Generator().manual_seed(77 + cout)
    wt = torch.randn((cout, 256, 1, 1), generator=g) / 16.0
    wt[0] = -wt[0].abs()                                   # a negative row
    if cout > 2:
        wt[1] *= 1e-6                                      # near-zero rows
        wt[cout - 1] *= 3e-5
    bias = (torch.arange(cout).float() - cout / 2) * 0.01
    return wt, bias


@pytest.fixture(scope="module")
def env(gpu_device):
    from deepemia_amd import _lib, p32
    dev = gpu_device
    g = torch.Generator().manual_seed(4242)
    wt = torch.randn((256, 256, 3, 3), generator=g) / 48.0
    bias = (torch.randperm(256, generator=g).float() - 127.5) / 256 * 0.2
    conv = make_layer(dev, wt, bias, 1)
    preds = {c: (predictor_weights(c), None) for c in COUTS}
    preds = {c: SimpleNamespace(wt=w, bias=b, L=make_layer(dev, w, b, 0)) for c, ((w, b), _) in preds.items()}
    xs = {}
    for name, (n, h, w, amps) in GEOS.items():
        x = torch.stack([torch.randn((h, w, 256), generator=g) * a for a in amps])
        xs[name] = SimpleNamespace(x=x, xp=p32.from_f32(x.to(dev), groups=n))
    yield SimpleNamespace(dev=dev, lib=_lib.load(), conv=conv, conv_wt=wt, conv_bias=bias, preds=preds, xs=xs, two={})


def launch(env, L, xp, n, h, w, act, out=None, out_meta=None, out_f32=False, tile=0, then=None, head_out=None, **over):
    from deepemia_amd import _lib
    d = _lib.ConvP32Desc(_lib.ptr(xp.buf), _lib.ptr(xp.meta), _lib.ptr(L.w3), _lib.ptr(L.scale3), _lib.ptr(L.bias), 0, 0,
                         _lib.ptr(out), _lib.ptr(out_meta), L.wbound, L.bbound, n, h, w, L.cin, h, w, L.cout, L.cout_pad, L.kh, L.kw,
                         1, L.pad, act, 0, 1 if out_f32 else 0, LD if out_f32 else 0, tile, 0, 0, _lib.ptr(head_out), 0, LD, 0,
                         n, h * w, 0, 0)
    if then is not None:
        d.head_planes, d.head_scale, d.head_bias, d.head_cout = _lib.ptr(then.w3), _lib.ptr(then.scale3), _lib.ptr(then.bias), then.cout
    for k, v in over.items():
        setattr(d, k, v)
    status = env.lib.demia_conv2d_p32(C.byref(d), int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return status


def canary(env, m):
    return torch.full(((m + 256), LD), CANARY32, dtype=torch.int32, device=env.dev)


def two_launches(env, geo, cout):
    """The planes layer, then the 1 x 1 layer (computed once per geometry and Cout, never changed): int32 view [M + 256, LD]."""
    from deepemia_amd import p32
    key = (geo, cout)
    if key not in env.two:
        n, h, w, _ = GEOS[geo]
        m = n * h * w
        t = p32.alloc((n, h, w, 256), env.dev, groups=n)
        assert launch(env, env.conv, env.xs[geo].xp, n, h, w, ACT_RELU, out=t.buf, out_meta=t.meta) == 0
        out = canary(env, m)
        assert launch(env, env.preds[cout].L, t, n, h, w, 0, out=out, out_f32=True) == 0
        env.two[key] = out
    return env.two[key]


def fused_launch(env, geo, cout, tile):
    n, h, w, _ = GEOS[geo]
    out = canary(env, n * h * w)
    assert launch(env, env.conv, env.xs[geo].xp, n, h, w, ACT_RELU, tile=tile, then=env.preds[cout].L, head_out=out) == 0
    return out


@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("tile", FUSED_TILES, ids=lambda t: f"t{t}")
@pytest.mark.parametrize("geo", list(GEOS))
def test_fused_equals_two_launches(env, geo, tile, cout):
    n, h, w, _ = GEOS[geo]
    m = n * h * w
    want = two_launches(env, geo, cout)
    got = fused_launch(env, geo, cout, tile)
    wf, gf = want[:m, :cout].view(torch.float32), got[:m, :cout].view(torch.float32)
    assert bool(torch.isfinite(wf).all()) and float(wf.abs().max()) > 0
    assert torch.equal(got[:m, :cout], want[:m, :cout]), f"{int((got[:m, :cout] != want[:m, :cout]).sum())} of {m * cout} differ, " \
        f"max |diff| {float((gf - wf).abs().max()):.3e}"
    assert bool((got[m:] == CANARY32).all()), "rows >= M written"
    assert bool((got[:m, cout:] == CANARY32).all()), "columns >= Cout written"
    assert bool((want[:m, cout:] == CANARY32).all())


@pytest.mark.parametrize("tile", FUSED_TILES, ids=lambda t: f"t{t}")
def test_fused_against_f64(env, tile):
    geo, cout = "3x13x13", 15
    n, h, w, _ = GEOS[geo]
    m = n * h * w
    c1 = S.Case(geo="rpnconv", cin=256, cout=256, k=3, stride=1, pad=1, h=h, w=w, res=S.RES_NONE, relu=True, rows="images")
    c2 = S.Case(geo="rpnpred", cin=256, cout=cout, k=1, stride=1, pad=0, h=h, w=w, res=S.RES_NONE, relu=False, rows="images", out_f32=True, out_ld=LD)
    t = S.reference(c1, dict(x=env.xs[geo].x, wt=env.conv_wt, scale=torch.ones(256), bias=env.conv_bias, res=None))
    pr = env.preds[cout]
    ref = S.reference(c2, dict(x=t.view(n, h, w, 256), wt=pr.wt, scale=torch.ones(cout), bias=pr.bias, res=None))
    got = fused_launch(env, geo, cout, tile)[:m, :cout].view(torch.float32).cpu()
    err = S.normalised_error(got, ref)
    print(f"fused RPN head, tile {tile}: normalised error against f64 {err:.3e} (bar {S.BAR:.0e})")
    assert err <= S.BAR


def test_fused_launch_refuses_what_it_cannot_do(env):
    geo, cout = "3x13x13", 15
    n, h, w, _ = GEOS[geo]
    pr = env.preds[cout].L
    for over in (dict(head_cout=17), dict(head_cout=0), dict(head_ld=8), dict(out_f32=1), dict(head_n=2), dict(Cout=224), dict(single=1)):
        out = canary(env, n * h * w)
        status = launch(env, env.conv, env.xs[geo].xp, n, h, w, ACT_RELU, then=pr, head_out=out, **over)
        assert status == DEMIA_EINVAL, over
        assert bool((out == CANARY32).all()), over


def test_engine_rpn_fused_equals_two_launches(gpu_device):
    from deepemia_amd import synth
    from deepemia_amd.engine import MaskRCNNEngine
    eng = MaskRCNNEngine(synth.random_d2_state_dict(50, 2, seed=0), 50, 2, 0.3, gpu_device, "f16x2")
    assert eng.rpn_fused and not eng.rpn_conv.single and not eng.rpn_pred.single
    img = torch.from_numpy(synth.em_tile(7, 256))[None].to(gpu_device)

    def rpn_of(raw):
        d = raw.dbg
        c = int(d["pcount"][0])
        return ([hd[..., :15].clone() for hd in d["heads"]], d["props"][0, :c].clone(), d["pscores"][0, :c].clone(), c)

    def outputs_of(raw):
        c = int(raw.count[0])
        return c, raw.boxes[0, :c].clone(), raw.scores[0, :c].clone(), raw.classes[0, :c].clone(), raw.packed[0, :c].clone()

    eager = eng.forward(img, keep_intermediates=True)
    torch.cuda.synchronize()
    heads_f, props_f, scores_f, count_f = rpn_of(eager)
    out_eager = outputs_of(eager)
    assert count_f > 0 and [tuple(hd.shape[1:3]) for hd in heads_f] == [(200, 200), (100, 100), (50, 50), (25, 25), (13, 13)]
    eng.forward_graphed(img)
    replay = eng.forward_graphed(img)                      # the second slot's graph
    torch.cuda.synchronize()
    for a, b in zip(out_eager, outputs_of(replay)):
        assert a == b if isinstance(a, int) else torch.equal(a, b)
    eng.release_cached_shapes()
    eng.rpn_fused = False
    two = eng.forward(img, keep_intermediates=True)
    torch.cuda.synchronize()
    heads_2, props_2, scores_2, count_2 = rpn_of(two)
    assert count_2 == count_f
    for a, b in zip(heads_f, heads_2):
        assert torch.equal(a, b)
    assert torch.equal(props_f, props_2) and torch.equal(scores_f, scores_2)
    for a, b in zip(out_eager, outputs_of(two)):
        assert a == b if isinstance(a, int) else torch.equal(a, b)
