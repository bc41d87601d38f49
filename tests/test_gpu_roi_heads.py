"""The ROI heads at one to eight classes against float64 references on the CPU.

The class count comes from the dataset; every other GPU module runs K = 2.  Here the heads run at K = 1 .. 8, which reaches
every code path that depends on it:
  * the fused deconv + class predictor of the f16x2 mask head (``conv_p32(..., head=...)``): the direct epilogue for
    K <= 2, the general one (LDS image, butterfly) for K = 3 and 4, on all three head tiles (tile hints 1, 2, anything
    else = 256 x 256, 128 x 256, 192 x 256);
  * the unfused mask head (K >= 5 on f16x2, every K on the exact-f32 engine): deconv planes, then ``mask_pred`` with
    ACT_SIGMOID into an f32 tensor of ``(K + 3) // 4 * 4`` columns;
  * the box head: fc1's 392 K-steps (Cin = 12544), fc2, and ``box_pred`` (5 K + 1 outputs, padded ``ld``);
  * detections and paste, which read class columns with a K-dependent stride;
  * the whole predictor against the oracle.

References are float64 torch on the CPU, computed from the operands the kernels see: the dequantised P32 input
(``p32.to_f32``) and the exact f32 weights of the state dict.  Stage calls run on engines that never ran a forward, so
every output is a fresh allocation.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

THR = 0.3
D = 100                          # detections per image = mask-head rows per image
CELLS = 196                      # 14 x 14 mask-head pixels per detection
MASK_GAIN, MASK_BIAS = 8.0, 0.5  # stage tests: class logits spread over a few units, sigmoids not saturated
E2E_SEEDS = {1: 0, 3: 0, 4: 7, 5: 5}  # end to end: per K a weight seed at which the oracle detects every class on em_tile(0, 1024)


@pytest.fixture(scope="module")
def heads(gpu_device):
    """Engines for stage calls (one per class count and precision, built on first use, never run a forward) and a cache
    for the float64 references that several parametrisations share."""
    from deepemia_amd import synth
    from deepemia_amd.engine import MaskRCNNEngine

    sds, engines = {}, {}

    def sd(k):
        if k not in sds:
            sds[k] = distinct_biases(synth.random_d2_state_dict(50, k, seed=0, mask_gain=MASK_GAIN, mask_bias=MASK_BIAS), k)
        return sds[k]

    def engine(k, prec="f16x2"):
        if (k, prec) not in engines:
            engines[(k, prec)] = MaskRCNNEngine(sd(k), 50, k, THR, gpu_device, prec)
        return engines[(k, prec)]

    yield dict(dev=gpu_device, sd=sd, engine=engine, cache={})
    engines.clear()


def distinct_biases(sd, k):
    """``random_d2_state_dict`` zeroes the biases of the head layers and gives the mask predictor the same bias for every
    class, so a bias read from the wrong row or column would go unseen.  Distinct values instead: the class-count
    independent layers (mask convs, deconv, fc1, fc2) from one generator -- fc1 / fc2 stay the same for every K -- and the
    class layers from one per K, the predictor's biases 0.8 apart in shuffled order."""
    g = torch.Generator().manual_seed(500)
    mh, bh, bp = "roi_heads.mask_head.", "roi_heads.box_head.", "roi_heads.box_predictor."
    for i in range(1, 5):
        sd[f"{mh}mask_fcn{i}.bias"] = torch.randn(256, generator=g) * 0.1
    sd[mh + "deconv.bias"] = torch.randn(256, generator=g) * 0.2
    sd[bh + "fc1.bias"] = torch.randn(1024, generator=g) * 0.1
    sd[bh + "fc2.bias"] = torch.randn(1024, generator=g) * 0.1
    gk = torch.Generator().manual_seed(600 + k)
    spread = 0.8 * (torch.arange(k, dtype=torch.float32) - (k - 1) / 2)
    sd[mh + "predictor.bias"] = MASK_BIAS + spread[torch.randperm(k, generator=gk)] + torch.randn(k, generator=gk) * 0.1
    sd[bp + "cls_score.bias"] = torch.randn(k + 1, generator=gk) * 0.5
    sd[bp + "bbox_pred.bias"] = torch.randn(4 * k, generator=gk) * 0.1
    return sd


def cached(heads, key, make):
    c = heads["cache"]
    if key not in c:
        c[key] = make()
    return c[key]


def f64(t):
    return t.detach().cpu().double()


def mask_head_weights(sd):
    """Deconv [Cin, Cout, 2, 2] as four [Cin, Cout] matrices (sub = dy * 2 + dx), its bias, the predictor [K, 256] and its
    bias, all float64, and the largest L1 norm of a predictor row."""
    mh = "roi_heads.mask_head."
    wd = sd[mh + "deconv.weight"].double()
    wsub = wd.permute(2, 3, 0, 1).reshape(4, 256, 256)
    wp = sd[mh + "predictor.weight"].double().reshape(-1, 256)
    return wsub, sd[mh + "deconv.bias"].double(), wp, sd[mh + "predictor.bias"].double(), float(wp.abs().sum(1).max())


def fused_head_reference(x, wsub, bd, wp, bp, relu=True):
    """f64 ``sigmoid(relu(x @ Wd_sub + bd) @ Wp.T + bp)`` in the kernel's output layout: row m * 4 + sub, column j.
    Returns (probabilities [4 M, K], max |deconv output|)."""
    m = x.shape[0]
    p = torch.empty((m, 4, wp.shape[0]), dtype=torch.float64)
    zmax = 0.0
    for s in range(4):
        z = x @ wsub[s] + bd
        if relu:
            z = z.clamp(min=0)
        zmax = max(zmax, float(z.abs().max()))
        p[:, s] = torch.sigmoid(z @ wp.T + bp)
    return p.reshape(4 * m, -1), zmax


def head_arg(eng, act):
    return (eng.mask_pred_w32, eng.mask_pred_b32, (eng.K + 3) // 4 * 4, act)


# ------------------------------------------------------------------------------------------------------------------
# 1. the fused deconv + class predictor, one launch
# ------------------------------------------------------------------------------------------------------------------
AMPS = (1.0, 0.01, 1.0)          # per-image amplitudes: neighbouring scale groups 100x apart


def fused_case(heads, k, b):
    """Input P32 [M, 1, 1, 256] (M = b * 100 * 196 rows, one scale group per image; b = 0: a ragged M of 333 rows, one
    group) and the f64 reference with its bar.  Also checks that the reference can tell a swapped head row, head biases
    shifted by one row, a missing deconv bias and a missing ReLU from the right answer at 100x the bar."""
    def make():
        from deepemia_amd import p32

        m = b * D * CELLS if b else 333
        g = torch.Generator().manual_seed(100 * k + b)
        x = torch.randn((m, 256), generator=g)
        if b:
            x = x * torch.tensor(AMPS[:b]).repeat_interleave(D * CELLS)[:, None]
        xp = p32.from_f32(x.to(heads["dev"]), groups=max(b, 1)).view(m, 1, 1, 256)
        xd = f64(p32.to_f32(xp)).reshape(m, 256)
        wsub, bd, wp, bp, l1 = mask_head_weights(heads["sd"](k))
        ref, zmax = fused_head_reference(xd, wsub, bd, wp, bp)
        tol = 0.25 * 2e-5 * zmax * l1 + 1e-7
        for i in range(k):
            for j in range(i + 1, k):
                assert float((ref[:, i] - ref[:, j]).abs().max()) > 100 * tol, (i, j)
        wrong = [fused_head_reference(xd, wsub, bd, wp, bp, relu=False)[0], fused_head_reference(xd, wsub, 0 * bd, wp, bp)[0]]
        if k > 1:
            wrong.append(fused_head_reference(xd, wsub, bd, wp, bp.roll(1))[0])
        for w in wrong:
            assert float((w - ref).abs().max()) > 100 * tol
        return x, xp, ref, tol
    return cached(heads, ("fused", k, b), make)


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("tile", [1, 2, 4])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_fused_mask_predictor_epilogue_vs_f64(heads, k, tile, b):
    """``conv_p32(deconv, ReLU, head=(predictor, sigmoid))`` -- K <= 2: the direct epilogue, K = 3, 4: the general one --
    on each head tile, one and three images per launch (19 600 rows per scale group: no multiple of 128, 192 or 256, so
    tiles straddle groups 100x apart).  Bar: the conv bar (2e-5 of max |deconv out|) through the 256-wide head dot
    (max_j sum |Wp_j|) and the sigmoid's slope (1/4), about 1e-3 here; observed at most 5.2e-7 at every K, tile and b.
    K = 2 and 3: every image of the three-image launch equals, bit for bit, the same image launched alone."""
    from deepemia_amd import p32
    from deepemia_amd._lib import ACT_RELU, ACT_SIGMOID

    eng = heads["engine"](k)
    x, xp, ref, tol = fused_case(heads, k, b)
    out = eng.conv_p32(xp, eng.deconv, act=ACT_RELU, tile_hint=tile, head=head_arg(eng, ACT_SIGMOID))
    assert tuple(out.shape) == (4 * xp.pixels, (k + 3) // 4 * 4)
    got = f64(out[:, :k])
    assert bool(torch.isfinite(got).all())
    err = float((got - ref).abs().max())
    assert err <= tol, (err, tol)
    if b == 3 and k in (2, 3):
        rows = D * CELLS
        for i in range(b):
            xi = p32.from_f32(x[i * rows:(i + 1) * rows].to(heads["dev"])).view(rows, 1, 1, 256)
            oi = eng.conv_p32(xi, eng.deconv, act=ACT_RELU, tile_hint=tile, head=head_arg(eng, ACT_SIGMOID))
            assert torch.equal(oi[:, :k], out[4 * i * rows:4 * (i + 1) * rows, :k]), i


@pytest.mark.parametrize("tile", [1, 2, 4])
@pytest.mark.parametrize("k", [1, 3])
def test_fused_mask_predictor_on_a_ragged_row_count(heads, k, tile):
    """333 rows: no multiple of any head tile's 128, 192 or 256 rows (2.6 tiles of 128 rows, fewer than two of 192 or
    256).  Observed at most 3.3e-7 against a bar of 8e-4."""
    from deepemia_amd._lib import ACT_RELU, ACT_SIGMOID

    eng = heads["engine"](k)
    _, xp, ref, tol = fused_case(heads, k, 0)
    out = eng.conv_p32(xp, eng.deconv, act=ACT_RELU, tile_hint=tile, head=head_arg(eng, ACT_SIGMOID))
    err = float((f64(out[:, :k]) - ref).abs().max())
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("k", [2, 3])
def test_fused_mask_predictor_single_plane_is_the_high_plane_product(heads, k):
    """The flagged single-plane mask head (``single_stages=("mask_fcn", "deconv")``): one MFMA per product on the high
    planes.  Reference: the f64 deconv of exactly those operands (half(x s) / s per scale group, half(w 2^e) / 2^e), then
    the head; bar: the f32-accumulation bar of 3e-6 of max |z|, propagated like the two-plane bar (1.5e-4 .. 1.8e-4 here);
    observed at most 3.6e-7.  The two-plane reference lies four bars from the high-plane one (asserted: more than three)
    and the output 3.9 bars from the two-plane reference (asserted: more than two), so a launch that ignored ``single``
    fails."""
    from deepemia_amd import engine as E, p32
    from deepemia_amd._lib import ACT_RELU, ACT_SIGMOID

    eng, sd = heads["engine"](k), heads["sd"](k)
    _, xp, ref2, _ = fused_case(heads, k, 3)
    m = xp.pixels
    hi = xp.buf[p32.HEADER_HALFS:].view(m, 8, 2, 32)[:, :, 0, :].reshape(m, 256)
    s = xp.meta[:, 1].repeat_interleave(m // xp.groups)
    xh = f64(hi.float() / s[:, None])
    mh = "roi_heads.mask_head."
    wd = sd[mh + "deconv.weight"]
    wp32 = wd.permute(2, 3, 1, 0).reshape(1024, 1, 1, 256)           # the engine's packing: row (dy, dx, co), K = ci
    planes, sw = E.split2_f16_scaled(wp32.to(heads["dev"]))
    wh = f64(planes[0].float().reshape(1024, 256) / sw[:, None])
    _, bd, wp, bp, l1 = mask_head_weights(sd)
    ref, zmax = fused_head_reference(xh, wh.reshape(4, 256, 256).transpose(1, 2), bd, wp, bp)
    tol = 0.25 * 3e-6 * zmax * l1 + 1e-7
    assert float((ref2 - ref).abs().max()) > 3 * tol
    L = E.ConvLayer(**{**eng.deconv.__dict__, "single": 1})
    out = eng.conv_p32(xp, L, act=ACT_RELU, head=head_arg(eng, ACT_SIGMOID))
    got = f64(out[:, :k])
    err = float((got - ref).abs().max())
    assert err <= tol, (err, tol)
    assert float((got - ref2).abs().max()) > 2 * tol


def test_fused_head_with_five_rows_is_refused(heads):
    """The fused head holds at most four rows (K <= 4): a fifth is an error, not a computation."""
    from deepemia_amd._lib import ACT_RELU, ACT_SIGMOID, HipKernelError

    eng, dev = heads["engine"](2), heads["dev"]
    _, xp, _, _ = fused_case(heads, 2, 0)
    w5, b5 = torch.zeros((5, 256), device=dev), torch.zeros((5,), device=dev)
    with pytest.raises(HipKernelError, match="at most 4 rows"):
        eng.conv_p32(xp, eng.deconv, act=ACT_RELU, head=(w5, b5, 8, ACT_SIGMOID))


# ------------------------------------------------------------------------------------------------------------------
# 2. the whole mask head
# ------------------------------------------------------------------------------------------------------------------
def mask_head_case(heads, k):
    """Two images of 100 pooled 14 x 14 x 256 ROIs (P32, one scale group per image, amplitudes 1 and 0.25) and the f64
    mask head on the dequantised values for ALL K class channels: four 3x3 convs + ReLU, the stride-2 deconv + ReLU, the
    1x1 predictor, sigmoid -> [200, K, 28, 28], with the bar."""
    def make():
        from deepemia_amd import p32

        g = torch.Generator().manual_seed(200 + k)
        x = torch.randn((2, D, 14, 14, 256), generator=g)
        x[1] *= 0.25
        xp = p32.from_f32(x.to(heads["dev"]), groups=2)
        xd = p32.to_f32(xp)
        sd = heads["sd"](k)
        mh = "roi_heads.mask_head."
        y = f64(xd).reshape(2 * D, 14, 14, 256).permute(0, 3, 1, 2)
        for i in range(1, 5):
            y = F.relu(F.conv2d(y, sd[f"{mh}mask_fcn{i}.weight"].double(), sd[f"{mh}mask_fcn{i}.bias"].double(), padding=1))
        z = F.relu(F.conv_transpose2d(y, sd[mh + "deconv.weight"].double(), sd[mh + "deconv.bias"].double(), stride=2))
        ref = torch.sigmoid(F.conv2d(z, sd[mh + "predictor.weight"].double(), sd[mh + "predictor.bias"].double()))
        l1 = float(sd[mh + "predictor.weight"].double().reshape(k, 256).abs().sum(1).max())
        tol = 0.25 * 5 * 2e-5 * float(z.abs().max()) * l1 + 1e-7
        return xp, xd, ref, tol
    return cached(heads, ("mask_head", k), make)


@pytest.mark.parametrize("k,prec", [(1, "f16x2"), (2, "f16x2"), (3, "f16x2"), (4, "f16x2"), (5, "f16x2"), (8, "f16x2"),
                                    (1, "f32"), (3, "f32"), (5, "f32")])
def test_mask_head_vs_f64_for_every_class(heads, k, prec):
    """``engine.mask_head`` -- f16x2: fused direct (K <= 2), fused general (K = 3, 4), unfused ACT_SIGMOID (K >= 5);
    exact f32: unfused at every K -- against the oracle's mask head restated for all class channels, de-blocked from
    ``[(roi * 196 + cell) * 4 + sub, ld]`` to ``[roi, K, 28, 28]``.  Bar: five GEMMs, each within 2e-5 of its max |out|,
    give at most 5 x 2e-5 of max |deconv out|, propagated as in the fused-head test through the predictor (max_j sum
    |Wp_j|) and the sigmoid (1/4): about 5e-3 in probability.  Observed at most 2.3e-6 (f16x2) and 3.4e-6 (f32)."""
    eng = heads["engine"](k, prec)
    xp, xd, ref, tol = mask_head_case(heads, k)
    x = xp if prec == "f16x2" else xd.contiguous()
    out = eng.mask_head(x)
    ld = (k + 3) // 4 * 4
    assert tuple(out.shape) == (2 * D * CELLS * 4, 1, 1, ld)
    got = f64(out).view(2 * D, 14, 14, 2, 2, ld)[..., :k].permute(0, 5, 1, 3, 2, 4).reshape(2 * D, k, 28, 28)
    assert bool(torch.isfinite(got).all())
    err = float((got - ref).abs().max())
    assert err <= tol, (err, tol)


# ------------------------------------------------------------------------------------------------------------------
# 3. the box head
# ------------------------------------------------------------------------------------------------------------------
BOX_CASES = {"b1": (1, None), "b3": (3, None), "count": (2, 613)}   # images, proposals of image 1 (rows beyond: zero, as ROIAlign leaves them)


def box_head_case(heads, case):
    """Pooled ROIs (b, 1000, 7, 7, 256) as P32 (one scale group per image) and their dequantised values, with the f64
    fc1 + ReLU, fc2 + ReLU on the NCHW-flattened rows -- the same for every K (the generator draws the fc weights before
    the class-count dependent ones)."""
    def make():
        from deepemia_amd import p32

        b, count = BOX_CASES[case]
        g = torch.Generator().manual_seed(300)
        x = torch.randn((3, 1000, 7, 7, 256), generator=g) * torch.tensor([1.0, 0.5, 2.0]).view(3, 1, 1, 1, 1)
        x = x[:b].contiguous()
        if count is not None:
            x[1, count:] = 0.0
        xp = p32.from_f32(x.to(heads["dev"]), groups=b)
        xd = p32.to_f32(xp)
        sd = heads["sd"](1)
        bh = "roi_heads.box_head."
        h = f64(xd).permute(0, 1, 4, 2, 3).reshape(b * 1000, 12544)
        h = F.relu(F.linear(h, sd[bh + "fc1.weight"].double(), sd[bh + "fc1.bias"].double()))
        h = F.relu(F.linear(h, sd[bh + "fc2.weight"].double(), sd[bh + "fc2.bias"].double()))
        return xp, xd, h
    return cached(heads, ("box_head", case), make)


@pytest.mark.parametrize("prec", ["f16x2", "f32"])
@pytest.mark.parametrize("k", [1, 2, 3, 5])
@pytest.mark.parametrize("case", list(BOX_CASES))
def test_box_head_vs_f64_per_block(heads, case, k, prec):
    """``engine.box_head``: fc1 (Cin 12544 = 392 K-steps, weights permuted from NCHW to NHWC flattening), fc2, and
    ``box_pred`` into ``(5 K + 1 + 3) // 4 * 4`` columns.  The class logits (columns 0 .. K) and the deltas (K + 1 .. 5 K)
    are each within 1e-4 of their OWN block's max |ref|: the deltas are ~10x smaller, one global max would hide them.
    Observed at most 2.9e-6 (logits) and 2.9e-6 (deltas) on both engines."""
    eng, sd = heads["engine"](k, prec), heads["sd"](k)
    xp, xd, h = box_head_case(heads, case)
    for key in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"):
        assert torch.equal(sd["roi_heads.box_head." + key], heads["sd"](1)["roi_heads.box_head." + key]), key
    bp = "roi_heads.box_predictor."
    logits = F.linear(h, sd[bp + "cls_score.weight"].double(), sd[bp + "cls_score.bias"].double())
    deltas = F.linear(h, sd[bp + "bbox_pred.weight"].double(), sd[bp + "bbox_pred.bias"].double())
    b = BOX_CASES[case][0]
    out = eng.box_head(xp if prec == "f16x2" else xd.contiguous())
    ld = (5 * k + 1 + 3) // 4 * 4
    assert tuple(out.shape) == (b, 1000, ld)
    got = f64(out).reshape(b * 1000, ld)
    for name, g, r in (("logits", got[:, :k + 1], logits), ("deltas", got[:, k + 1:5 * k + 1], deltas)):
        assert bool(torch.isfinite(g).all()), name
        err = float((g - r).abs().max() / r.abs().max())
        assert err <= 1e-4, (name, err)


# ------------------------------------------------------------------------------------------------------------------
# 4. paste at other class counts
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 5])
def test_paste_reads_the_detections_class_column(heads, k):
    """``demia_paste_masks`` on the hand-blocked layout ``[(det * 196 + cell) * 4 + sub, ld]`` with ``ld = (K + 3) // 4 * 4``:
    each detection's own class column holds a blob, every other class column -1 (reading the wrong one empties the mask).
    Against the oracle's paste of the blobs: IoU >= 0.999, at most a threshold-tie pixel per instance, no empty mask."""
    from oracle import maskrcnn_ref as R

    eng, dev = heads["engine"](k, "f32"), heads["dev"]
    g = torch.Generator().manual_seed(400 + k)
    size, n = 320, 37
    ld = (k + 3) // 4 * 4
    yy, xx = torch.meshgrid(torch.arange(28.0), torch.arange(28.0), indexing="ij")
    c = torch.rand((n, 2), generator=g) * 12 + 8
    sig = torch.rand((n,), generator=g) * 5 + 4
    mp = torch.exp(-((yy - c[:, 0, None, None]) ** 2 + (xx - c[:, 1, None, None]) ** 2) / (2 * sig[:, None, None] ** 2))
    classes = torch.randint(0, k, (n,), generator=g, dtype=torch.int32)
    classes[:k] = torch.arange(k, dtype=torch.int32)                       # every class occurs
    blocked = torch.full((D, CELLS, 4, ld), 7.0)                            # padding columns: a read of one fills the box
    for dy in range(2):
        for dx in range(2):
            sub = mp[:, dy::2, dx::2].reshape(n, CELLS)
            for cl in range(k):
                blocked[:n, :, dy * 2 + dx, cl] = torch.where(classes[:, None] == cl, sub, torch.full_like(sub, -1.0))
    cxy = torch.rand((n, 2), generator=g) * (size - 60) + 30
    wh = torch.rand((n, 2), generator=g) * 80 + 20
    boxes = torch.zeros((1, D, 4))
    boxes[0, :n] = torch.cat([cxy - wh / 2, cxy + wh / 2], dim=1)
    det_classes = torch.zeros((1, D), dtype=torch.int32)
    det_classes[0, :n] = classes
    ob, valid, packed, _ = eng.paste(blocked.view(D * CELLS * 4, 1, 1, ld).to(dev), boxes.to(dev), det_classes.to(dev),
                                     torch.tensor([n], dtype=torch.int32, device=dev), size, size, size, size)
    assert bool(valid[0, :n].all())
    masks = eng.unpack(packed[0, :n].contiguous(), size, size).cpu()
    want = R.paste_masks(mp, ob[0, :n].cpu(), size, size)
    assert bool((want.sum((1, 2)) > 0).all()) and bool((masks.sum((1, 2)) > 0).all())
    inter = (masks & want).sum((1, 2)).float()
    union = (masks | want).sum((1, 2)).float().clamp(min=1)
    assert float((inter / union).min()) >= 0.999
    assert int((masks != want).sum()) <= n


# ------------------------------------------------------------------------------------------------------------------
# 5. end to end
# ------------------------------------------------------------------------------------------------------------------
def oracle_prediction(heads, k):
    def make():
        from deepemia_amd import synth
        from oracle import maskrcnn_ref as R

        sd = synth.random_d2_state_dict(50, k, seed=E2E_SEEDS[k])
        img = synth.em_tile(0, 1024)
        return sd, img, R.predict(img, sd, 50, THR)
    return cached(heads, ("e2e", k), make)


@pytest.mark.parametrize("prec", ["f16x2", "f32"])
@pytest.mark.parametrize("k", [1, 3, 4, 5])
def test_end_to_end_at_other_class_counts(heads, k, prec):
    """The whole predictor at K = 1, 3, 4 (fused general mask epilogue), 5 (unfused) against the oracle, with the bars of
    ``test_end_to_end_f32_matches_oracle``.  Weights ``random_d2_state_dict(50, K, seed=E2E_SEEDS[K])``: seeds 0, 0, 7, 5
    for K = 1, 3, 4, 5, chosen so that every class 0 .. K - 1 is among the oracle's 100 detections (at seed 0, class 3 of
    K = 4 and 5 never is) -- otherwise the test would prove nothing about class columns."""
    from deepemia_amd.engine import MaskRCNNEngine
    from deepemia_amd.predictor import Predictor

    sd, img, ref = oracle_prediction(heads, k)
    n = ref["scores"].shape[0]
    assert n >= 20 and set(ref["pred_classes"].tolist()) == set(range(k))
    eng = MaskRCNNEngine(sd, 50, k, THR, heads["dev"], prec)
    inst = Predictor(eng)(img)["instances"]
    assert len(inst) == n
    got = inst.to("cpu")
    np.testing.assert_array_equal(got.pred_classes.numpy(), ref["pred_classes"].numpy())
    assert float((got.scores - ref["scores"]).abs().max()) < 1e-4
    assert bool((got.scores[:-1] >= got.scores[1:]).all())
    assert float((got.pred_boxes - ref["pred_boxes"]).abs().max()) < 5e-2
    m, r = got.pred_masks, ref["pred_masks"]
    iou = (m & r).sum((1, 2)).float() / (m | r).sum((1, 2)).float().clamp(min=1)
    assert float(iou.min()) >= 0.999
    del inst, got, eng
