"""Sixteen-wave grids of the P32 convolution (tile id 1 at K >= 2304 and with the fused head; dev tile hints 61-64) against their
eight-wave twins (dev hint 65 = ``launch_q<2, 4, 4, 2>`` at any K; id 2), bit for bit.

A tile's wave grid decides which wave owns which 16 x 16 accumulator block, which DMA pieces it requests and which rows it takes
through the epilogue -- never the K order or the MFMA order of an output element.  So planes, ``out_meta`` (scale and atomic max)
and fused-head outputs of ``launch_q<4, 4, 2, 2>`` / ``<2, 8, 4, 1>`` (256 x 256) and ``<4, 4, 1, 2>`` / ``<2, 8, 2, 1>``
(128 x 256) must EQUAL those of ``<2, 4, 4, 2>`` / ``<2, 4, 2, 2>``.  The shapes are the smallest at which the per-wave
bookkeeping can go wrong: one partial tile with a single K-step; a ragged 3x3 with two column tiles, three scale groups whose
boundaries fall inside tiles, residual + ReLU and image amplitudes 100x apart; stride 2 with a nearest-2x residual; the fused head.

Needs the dev build of the library (``DEEPEMIA_DEV_LIB=1``); skipped otherwise, like the other dev-tile tests.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

# (sixteen-wave hint, eight-wave twin)
GRIDS = [(61, 65), (62, 65), (63, 2), (64, 2)]


def _dev():
    from conftest import needs_dev_build
    needs_dev_build("")


class _Layer:
    def __init__(self, cout, cin, k, seed, dev):
        from deepemia_amd import engine as E
        g = torch.Generator().manual_seed(seed)
        w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
        scale = 0.5 + torch.rand(cout, generator=g)
        bias = torch.randn(cout, generator=g) * 0.1
        planes, sw = E.split2_f16_scaled(w.permute(0, 2, 3, 1).contiguous().to(dev))
        self.cout, self.cin, self.k = cout, cin, k
        self.w = E.tile_weight_planes_p32(planes)
        self.scale = (scale.to(dev) / sw[:cout]).contiguous()
        self.bias = bias.to(dev).contiguous()
        self.wbound = float((scale.abs() * w.abs().flatten(1).sum(1)).max())
        self.bbound = float(bias.abs().max())


def _launch(x, L, stride, pad, act, res, res_mode, hint, head=None):
    """One ``demia_conv2d_p32`` launch; returns (planes, meta) or the fused head's f32 rows."""
    from deepemia_amd import _lib, p32
    lib = _lib.load()
    n, h, w, cin = x.shape
    ho, wo = (h + 2 * pad - L.k) // stride + 1, (w + 2 * pad - L.k) // stride + 1
    groups = x.groups
    dev = x.buf.device
    d = _lib.ConvP32Desc()
    d.in_, d.in_meta, d.w, d.scale, d.bias = _lib.ptr(x.buf), _lib.ptr(x.meta), _lib.ptr(L.w), _lib.ptr(L.scale), _lib.ptr(L.bias)
    if res is not None:
        d.residual, d.res_meta = _lib.ptr(res.buf), _lib.ptr(res.meta)
    d.wbound, d.bbound = L.wbound, L.bbound
    d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout, d.CoutPad = n, h, w, cin, ho, wo, L.cout, L.cout
    d.KH, d.KW, d.stride, d.pad, d.act, d.res_mode, d.tile_hint = L.k, L.k, stride, pad, act, res_mode, hint
    d.groups, d.group_rows, d.row0 = groups, (n * ho * wo) // groups, 0
    if head is None:
        out = p32.alloc((n, ho, wo, L.cout), dev, groups=groups)
        out.buf[p32.HEADER_HALFS:].fill_(float("nan"))           # every element must be written
        d.out, d.out_meta = _lib.ptr(out.buf), _lib.ptr(out.meta)
        ret = (out.buf, out.meta)
    else:
        hw, hb, hact = head
        hout = torch.full((n * ho * wo * (L.cout // 256), 2), float("nan"), dtype=torch.float32, device=dev)
        d.head_w, d.head_b, d.head_out, d.head_n, d.head_ld, d.head_act = _lib.ptr(hw), _lib.ptr(hb), _lib.ptr(hout), 2, 2, hact
        ret = (hout,)
    _lib.check(lib.demia_conv2d_p32(C.byref(d), int(torch.cuda.current_stream(dev).cuda_stream)), "demia_conv2d_p32")
    torch.cuda.synchronize()
    return ret


def _same(a, b):
    assert len(a) == len(b)
    for s, t in zip(a, b):
        assert not bool(torch.isnan(t.float()).any())
        assert torch.equal(s, t)


@pytest.mark.parametrize("sixteen,eight", GRIDS)
def test_one_partial_tile_one_k_step(gpu_device, sixteen, eight):
    """1x1, 32 -> 256 channels, M = 200: one workgroup, rows 200..255 gather the zero header, kloop = 1 (prologue DMA only)."""
    _dev()
    from deepemia_amd import p32
    from deepemia_amd._lib import ACT_NONE, RES_NONE
    g = torch.Generator().manual_seed(1)
    x = p32.from_f32((torch.randn(1, 10, 20, 32, generator=g) * 3.0).to(gpu_device))
    L = _Layer(256, 32, 1, 11, gpu_device)
    ref = _launch(x, L, 1, 0, ACT_NONE, None, RES_NONE, eight)
    assert float(ref[1][0, 0]) > 0.0
    _same(_launch(x, L, 1, 0, ACT_NONE, None, RES_NONE, sixteen), ref)


@pytest.mark.parametrize("sixteen,eight", GRIDS)
def test_ragged_three_groups_residual_relu(gpu_device, sixteen, eight):
    """3x3 pad 1, 64 -> 512 channels (two column tiles), three images of 14 x 14 (M = 588 = 2 x 256 + 76, 76 % 32 != 0), one scale
    group per image -- the boundaries at rows 196 and 392 fall inside tiles, off every 32-row block edge --, residual SAME + ReLU,
    image amplitudes 100x apart."""
    _dev()
    from deepemia_amd import p32
    from deepemia_amd._lib import ACT_RELU, RES_SAME
    g = torch.Generator().manual_seed(2)
    amp = torch.tensor([0.05, 5.0, 0.5]).view(3, 1, 1, 1)
    x = p32.from_f32((torch.randn(3, 14, 14, 64, generator=g) * amp).to(gpu_device), groups=3)
    res = p32.from_f32((torch.randn(3, 14, 14, 512, generator=g) * amp * 1.5).to(gpu_device), groups=3)
    L = _Layer(512, 64, 3, 12, gpu_device)
    ref = _launch(x, L, 1, 1, ACT_RELU, res, RES_SAME, eight)
    assert float(ref[1][:, 0].min()) > 0.0
    _same(_launch(x, L, 1, 1, ACT_RELU, res, RES_SAME, sixteen), ref)


@pytest.mark.parametrize("sixteen,eight", GRIDS)
def test_stride_two_nearest_2x_residual(gpu_device, sixteen, eight):
    """1x1 stride 2, 256 -> 256 channels, 2 x 25 x 25 -> 13 x 13 (M = 338), residual upsampled nearest-2x from 7 x 7."""
    _dev()
    from deepemia_amd import p32
    from deepemia_amd._lib import ACT_NONE, RES_UP2
    g = torch.Generator().manual_seed(3)
    x = p32.from_f32((torch.randn(2, 25, 25, 256, generator=g) * 2.0).to(gpu_device))
    res = p32.from_f32((torch.randn(2, 7, 7, 256, generator=g) * 2.0).to(gpu_device))
    L = _Layer(256, 256, 1, 13, gpu_device)
    ref = _launch(x, L, 2, 0, ACT_NONE, res, RES_UP2, eight)
    _same(_launch(x, L, 2, 0, ACT_NONE, res, RES_UP2, sixteen), ref)


def test_product_tile_at_large_k(gpu_device):
    """Tile id 1 as the product dispatches it at K >= 2304 (3x3, 256 -> 256 channels: 72 K-steps, sixteen waves of 128 x 32), two
    images of 14 x 14 in two scale groups (M = 392: one whole tile, one ragged), against the eight-wave twin."""
    _dev()
    from deepemia_amd import p32
    from deepemia_amd._lib import ACT_RELU, RES_NONE
    g = torch.Generator().manual_seed(5)
    x = p32.from_f32((torch.randn(2, 14, 14, 256, generator=g) * torch.tensor([3.0, 0.03]).view(2, 1, 1, 1)).to(gpu_device), groups=2)
    L = _Layer(256, 256, 3, 15, gpu_device)
    ref = _launch(x, L, 1, 1, ACT_RELU, None, RES_NONE, 65)
    assert float(ref[1][:, 0].min()) > 0.0
    for hint in (1, 62, 61):
        _same(_launch(x, L, 1, 1, ACT_RELU, None, RES_NONE, hint), ref)


@pytest.mark.parametrize("sixteen,eight", [(61, 65), (1, 65)])
def test_fused_head(gpu_device, sixteen, eight):
    """256 -> 1024 channels + ReLU with a 2-row head + sigmoid folded in, M = 392 (two row tiles x four column tiles): the head's
    f32 rows straight from the accumulators, partial sums of the WN waves added in wave order.  Only the 4 x 4 grid keeps WN and TN
    of the eight-wave tile and with them the order of that sum; the 2 x 8 grid has no fused-head instantiation."""
    _dev()
    from deepemia_amd import p32
    from deepemia_amd._lib import ACT_RELU, ACT_SIGMOID, RES_NONE
    g = torch.Generator().manual_seed(4)
    x = p32.from_f32((torch.randn(2, 14, 14, 256, generator=g) * 2.0).to(gpu_device))
    L = _Layer(1024, 256, 1, 14, gpu_device)
    hw = (torch.randn(2, 256, generator=g) * 0.1).to(gpu_device)
    hb = torch.randn(2, generator=g).to(gpu_device)
    ref = _launch(x, L, 1, 0, ACT_RELU, None, RES_NONE, eight, head=(hw, hb, ACT_SIGMOID))
    _same(_launch(x, L, 1, 0, ACT_RELU, None, RES_NONE, sixteen, head=(hw, hb, ACT_SIGMOID)), ref)
