"""What ``test_gpu_conv_p32_tiles.py`` sweeps and what it compares with, shared with ``test_cpu_conv_p32_tile_list.py``.

No GPU is needed for anything in here: the tile tables (restated from ``csrc/conv_p32.hip``, checked against the source by
the CPU module), the case list, the per-tile row counts, the seeded operands, the float64 reference with its deliberately
wrong variants, and a Python restatement of the launch-time tile choice (``choose_tile``).
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent.parent
SOURCE = ROOT / "deepemia_amd" / "csrc" / "conv_p32.hip"

BAR = 2e-5               # max-normalised error against f64: the bar of test_conv_p32_vs_torch
SINGLE_BAR = 3e-6        # single-plane compile against the f64 product of the high planes: test_single_plane_conv_...
TELL = 100.0             # a wrong reference must be further than TELL * BAR from the right one

# id -> (block rows bm, block columns bn)
PLANE_TILES: Dict[int, Tuple[int, int]] = {1: (256, 256), 2: (128, 256), 4: (192, 256), 12: (160, 256), 13: (224, 256),
                                           6: (256, 128), 7: (128, 128), 9: (256, 64), 11: (128, 64)}
GUARDED_TILES: Dict[int, Tuple[int, int]] = {7: (128, 128), 9: (256, 64), 10: (256, 64), 11: (128, 64)}
GUARDED_BY_HINT_ONLY = {10}          # never chosen by the model, never the fall-back of another hint: dead in the product


@dataclass(frozen=True)
class Tile:
    id: int
    guarded: bool

    @property
    def name(self) -> str:
        return f"{self.id}G" if self.guarded else str(self.id)

    @property
    def bm(self) -> int:
        return (GUARDED_TILES if self.guarded else PLANE_TILES)[self.id][0]

    @property
    def bn(self) -> int:
        return (GUARDED_TILES if self.guarded else PLANE_TILES)[self.id][1]


TILES: List[Tile] = [Tile(i, False) for i in PLANE_TILES] + [Tile(i, True) for i in GUARDED_TILES]


def tile_named(name: str) -> Tile:
    return next(t for t in TILES if t.name == name)


# ------------------------------------------------------------------------------------------------------------------
# the source's own tile lists
# ------------------------------------------------------------------------------------------------------------------
def _product_text() -> str:
    """conv_p32.hip without the regions only the dev build compiles (``#if P32_DEV_TILES`` / ``#if !P32_SINGLE && P32_DEV_TILES``)."""
    out, depth, skip_at = [], 0, None
    for line in SOURCE.read_text().splitlines():
        s = line.strip()
        if s.startswith("#if"):
            depth += 1
            if skip_at is None and re.match(r"#if\s+(!P32_SINGLE\s*&&\s*)?P32_DEV_TILES\b", s):
                skip_at = depth
        elif s.startswith("#endif"):
            if skip_at == depth:
                skip_at = None
                depth -= 1
                continue
            depth -= 1
        if skip_at is None:
            out.append(line)
    return "\n".join(out)


def parse_ktiles() -> Dict[int, Tuple[int, int]]:
    m = re.search(r"constexpr\s+TileCfg\s+kTiles\[\]\s*=\s*\{(.*?)\};", SOURCE.read_text(), re.S)
    assert m, "kTiles not found"
    return {int(a): (int(b), int(c)) for a, b, c in re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\}", m.group(1))}


def parse_dispatch() -> Tuple[Dict[int, Tuple[int, int]], Dict[int, Tuple[int, int]]]:
    """(straight-line, guarded) instantiations the product build dispatches to: ``case id: ... launch_q<WM, WN, TM, TN[, true, EPI]>``
    of the two switches behind the fused-head one; block = (WM * TM * 32, WN * TN * 32)."""
    text = _product_text()
    text = text[text.index("if (!planes) {"):]
    plain, guarded = {}, {}
    for cid, wm, wn, tm, tn, rest in re.findall(r"case\s+(\d+):[^\n]*?launch_q<\s*(\d+),\s*(\d+),\s*(\d+),\s*(\d+)([^>]*)>\(p, st\)", text):
        blk = (int(wm) * int(tm) * 32, int(wn) * int(tn) * 32)
        if "EPI_GENERIC" in rest:
            guarded[int(cid)] = blk
        else:
            assert rest.strip() == "", rest
            plain[int(cid)] = blk
    return plain, guarded


# ------------------------------------------------------------------------------------------------------------------
# launch-time decisions of demia_conv2d_p32, restated
# ------------------------------------------------------------------------------------------------------------------
def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def predict_us(bm: int, bn: int, m: int, cout_pad: int, ksteps: int, residual: bool) -> float:
    tiles = cdiv(m, bm) * (cout_pad // bn)
    smem = 2 * (bm + bn) * 128
    occ = 2 if 160 * 1024 // smem >= 2 else 1
    area = bm * bn / 65536.0
    step = 2.0 * area * (1.0 + 0.2 * (1.0 - area))
    edge = 6.0 + 6.0 * area * (1.5 if residual else 1.0)
    if occ == 1:
        return ((tiles + 255) // 256) * (ksteps * step + edge)
    return ((tiles + 511) // 512) * (2.0 * ksteps * step + 2.0 * 0.5 * edge)


def choose_tile(m: int, cout_pad: int, ksteps: int, residual: bool) -> int:
    best, best_t = 0, 1e30
    for tid, (bm, bn) in parse_ktiles().items():          # the source's order: ties go to the earlier entry
        if cout_pad % bn:
            continue
        t = predict_us(bm, bn, m, cout_pad, ksteps, residual)
        if t < best_t:
            best, best_t = tid, t
    return best


def resolve(hint: int, m: int, cin: int, cout: int, k: int, residual: bool, out_f32: bool) -> Optional[str]:
    """The kernel a (hint, layer) pair runs: a tile name (``"7G"`` = guarded epilogue), or None where the entry point refuses."""
    cout_pad = cdiv(cout, 64) * 64
    tile = hint or choose_tile(m, cout_pad, k * k * cin // 32, residual)
    bn = 64 if tile in (9, 10, 11) else (128 if tile in (6, 7) else 256)
    if out_f32 or cout % bn:
        if tile not in (7, 9, 10, 11):
            tile = 7 if cout_pad % 128 == 0 else 11
        return None if tile == 7 and cout_pad % 128 else f"{tile}G"
    if tile not in PLANE_TILES or cout_pad % bn:
        return None
    return str(tile)


def r101_layers(images: int) -> List[Tuple[int, int, int, int, bool, bool]]:
    """(M, Cin, Cout, k, residual, out_f32) of every demia_conv2d_p32 launch but the fused mask head in one R101-FPN forward of
    ``images`` 800 x 800 inputs (1000 proposals, 100 detections per image, two classes)."""
    out = []
    hw, cin = 200, 64
    for stage, (blocks, mid) in enumerate(((3, 64), (4, 128), (23, 256), (3, 512))):
        for b in range(blocks):
            stride = 2 if (b == 0 and stage > 0) else 1
            hw //= stride
            m = images * hw * hw
            if b == 0:
                out.append((m, cin, mid * 4, 1, False, False))
            out += [(m, cin, mid, 1, False, False), (m, mid, mid, 3, False, False), (m, mid, mid * 4, 1, True, False)]
            cin = mid * 4
    for lvl, (s, c) in enumerate(((25, 2048), (50, 1024), (100, 512), (200, 256))):
        out += [(images * s * s, c, 256, 1, lvl > 0, False), (images * s * s, 256, 256, 3, False, False)]
    for s in (200, 100, 50, 25, 13):
        out += [(images * s * s, 256, 256, 3, False, False), (images * s * s, 256, 15, 1, False, True)]
    out += [(images * 1000, 12544, 1024, 1, False, False), (images * 1000, 1024, 1024, 1, False, False), (images * 1000, 1024, 11, 1, False, True)]
    out += [(images * 100 * 196, 256, 256, 3, False, False)] * 4
    return out


def auto_tiles(images: int) -> Dict[str, int]:
    hist: Dict[str, int] = {}
    for m, cin, cout, k, res, f32 in r101_layers(images):
        name = resolve(0, m, cin, cout, k, res, f32)
        hist[name] = hist.get(name, 0) + 1
    return dict(sorted(hist.items(), key=lambda kv: -kv[1]))


# ------------------------------------------------------------------------------------------------------------------
# the sweep
# ------------------------------------------------------------------------------------------------------------------
RES_NONE, RES_SAME, RES_UP2 = 0, 1, 2


@dataclass(frozen=True)
class Case:
    geo: str
    cin: int
    cout: int
    k: int
    stride: int
    pad: int
    h: int
    w: int
    res: int
    relu: bool
    rows: str            # how the row count follows the tile: "partial" (M = bm - 37: one partial tile), "exact" (M = j * bm),
                         # "fixed" (n_min rows), "images" (n >= n_min whole images), "many" (M = j * bm - 45, at least 520 tiles)
    n_min: int = 1
    out_f32: bool = False
    out_ld: int = 0
    amp_exp: int = 0     # activations are N(0, 1) * 10^amp_exp

    @property
    def name(self) -> str:
        return f"{self.geo}-o{self.cout}" + ("f" if self.out_f32 else "")

    @property
    def cout_pad(self) -> int:
        return cdiv(self.cout, 64) * 64

    @property
    def ho(self) -> int:
        return (self.h + 2 * self.pad - self.k) // self.stride + 1

    @property
    def wo(self) -> int:
        return (self.w + 2 * self.pad - self.k) // self.stride + 1

    @property
    def guarded(self) -> bool:
        return self.out_f32 or self.cout % 64 != 0

    @property
    def ld(self) -> int:
        return self.out_ld or self.cout


def _geo(geo, couts, **kw):
    return [Case(geo=geo, cout=c, out_f32=f, out_ld=ld, **kw) for c, f, ld in couts]


P, F32 = False, True
CASES: List[Case] = (
    # 1x1, Cin = 32: a single K-step, the two-stage pipeline has no steady state; one partial tile
    _geo("k1c32", [(256, P, 0), (128, P, 0), (64, P, 0), (15, F32, 16), (80, F32, 0)],
         cin=32, k=1, stride=1, pad=0, h=1, w=1, res=RES_NONE, relu=True, rows="partial", amp_exp=-3)
    # 1x1, Cin = 96: three K-steps (odd), same-shape residual; whole tiles exactly
    + _geo("k1c96same", [(512, P, 0), (384, P, 0), (192, P, 0), (96, P, 0)],
           cin=96, k=1, stride=1, pad=0, h=1, w=1, res=RES_SAME, relu=False, rows="exact", amp_exp=3)
    # 1x1, stride 2, Cin = 256, odd H and W
    + _geo("k1s2c256", [(256, P, 0), (128, P, 0), (80, F32, 0), (15, F32, 16)],
           cin=256, k=1, stride=2, pad=0, h=37, w=41, res=RES_NONE, relu=True, rows="images", amp_exp=-2)
    # 3x3, pad 1, Cin = 64, three images or more: halo rows gather across image boundaries and the zero header
    + _geo("k3c64n3", [(256, P, 0), (64, P, 0), (96, P, 0), (32, P, 0)],
           cin=64, k=3, stride=1, pad=1, h=13, w=11, res=RES_NONE, relu=False, rows="images", n_min=3, amp_exp=2)
    # 3x3, stride 2, pad 1, Cin = 128, odd H and W
    + _geo("k3s2c128", [(512, P, 0), (192, P, 0), (80, F32, 0)],
           cin=128, k=3, stride=2, pad=1, h=33, w=31, res=RES_NONE, relu=True, rows="images", amp_exp=-1)
    # 1x1, Cin = 512, nearest-2x residual, odd Ho and Wo: the FPN lateral
    + _geo("k1c512up2", [(256, P, 0), (384, P, 0), (96, P, 0), (32, P, 0)],
           cin=512, k=1, stride=1, pad=0, h=25, w=27, res=RES_UP2, relu=False, rows="images", amp_exp=1)
    # 3x3, Cin = 256: 72 K-steps, the FPN-output and mask-head shape
    + _geo("k3c256", [(256, P, 0), (128, P, 0), (15, F32, 16), (96, P, 0)],
           cin=256, k=3, stride=1, pad=1, h=14, w=14, res=RES_NONE, relu=True, rows="images", amp_exp=0)
    # H = W = 1, Cin = 1024, N = 700: the fully-connected shape
    + _geo("fc", [(512, P, 0), (64, P, 0), (80, F32, 0)],
           cin=1024, k=1, stride=1, pad=0, h=1, w=1, res=RES_NONE, relu=True, rows="fixed", n_min=700, amp_exp=-3)
    # many workgroups: 1x1, Cin = 64, at least 520 tiles of the swept shape -- more than one round at two workgroups per CU
    + _geo("many", [(256, P, 0), (96, P, 0)],
           cin=64, k=1, stride=1, pad=0, h=1, w=1, res=RES_NONE, relu=True, rows="many", amp_exp=3)
)


def runs_on(tile: Tile, case: Case) -> bool:
    """Is (tile, case) part of the sweep?  Straight-line tiles take whole column tiles of planes; guarded tiles take the
    guarded cases -- including the ones the entry point refuses (7G at CoutPad % 128 != 0), which the sweep asserts and skips."""
    if tile.guarded != case.guarded:
        return False
    return tile.guarded or case.cout % tile.bn == 0


def refused(tile: Tile, case: Case) -> bool:
    return case.cout_pad % tile.bn != 0


def nwg(tile: Tile, case: Case, n: int) -> int:
    return cdiv(n * case.ho * case.wo, tile.bm) * (case.cout_pad // tile.bn)


def _candidates(tile: Tile, case: Case) -> List[int]:
    ntn = max(1, case.cout_pad // tile.bn)
    if case.rows == "partial":
        return [tile.bm - 37]
    if case.rows == "fixed":
        return [case.n_min]
    if case.rows == "exact":
        return [j * tile.bm for j in range(1, 17)]
    if case.rows == "many":
        return [j * tile.bm - 45 for j in range(cdiv(520, ntn), cdiv(520, ntn) + 8)]
    return list(range(case.n_min, case.n_min + 4096 // (case.ho * case.wo) + 1))


def _plan() -> Dict[Tuple[str, str], int]:
    """Rows (images) per (tile, case): walking the cases in order, each takes the smallest row count of its rule whose
    workgroup count lands on a residue mod 8 that the tile has not seen yet (else the smallest).  Pure arithmetic, so the
    plan is the same on every machine; the CPU module asserts that every tile ends up with all eight residues."""
    plan = {}
    for tile in TILES:
        seen = set()
        mine = [c for c in CASES if runs_on(tile, c) and not refused(tile, c)]
        for case in sorted(mine, key=lambda c: len(_candidates(tile, c)) > 1):      # the rules without a choice first
            cand = _candidates(tile, case)
            n = next((n for n in cand if nwg(tile, case, n) % 8 not in seen), cand[0])
            seen.add(nwg(tile, case, n) % 8)
            plan[(tile.name, case.name)] = n
    return plan


PLAN = _plan()
SWEEP: List[Tuple[Tile, Case]] = [(t, c) for t in TILES for c in CASES if runs_on(t, c)]


def rows_for(tile: Tile, case: Case) -> int:
    """Images (= rows for the H = W = 1 geometries) of this (tile, case); a refused pair gets the rule's smallest count."""
    return PLAN.get((tile.name, case.name), _candidates(tile, case)[0])


def n_common(case: Case) -> int:
    """Images of the launches that are compared between tiles (and the size the operands are generated at)."""
    return max(n for (t, c), n in PLAN.items() if c == case.name)


# ------------------------------------------------------------------------------------------------------------------
# operands and the float64 reference
# ------------------------------------------------------------------------------------------------------------------
def operands(case: Case, n: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """Seeded f32 operands of ``n`` images (default: all the sweep needs): x NHWC with amplitude 10^amp_exp, weights
    [Cout, Cin, k, k] of unit output variance, a FrozenBN-style scale in [0.5, 1.5], distinct biases and the residual (both of
    the output's amplitude)."""
    n = n or n_common(case)
    g = torch.Generator().manual_seed(1000 + CASES.index(case))
    amp = 10.0 ** case.amp_exp
    wt = torch.randn((case.cout, case.cin, case.k, case.k), generator=g) / (case.cin * case.k * case.k) ** 0.5
    scale = torch.rand((case.cout,), generator=g) + 0.5
    bias = (torch.randperm(case.cout, generator=g).float() - (case.cout - 1) / 2) / case.cout * (0.6 * amp)
    ops = dict(wt=wt, scale=scale, bias=bias, res=None)
    gx = torch.Generator().manual_seed(5000 + CASES.index(case))
    gr = torch.Generator().manual_seed(9000 + CASES.index(case))
    ops["x"] = torch.stack([torch.randn((case.h, case.w, case.cin), generator=gx) for _ in range(n)]) * amp if case.h * case.w > 1 \
        else (torch.randn((n, case.cin), generator=gx) * amp).view(n, 1, 1, case.cin)
    if case.res == RES_SAME:
        ops["res"] = (torch.randn((n, case.ho * case.wo * case.cout), generator=gr) * amp).view(n, case.ho, case.wo, case.cout)
    elif case.res == RES_UP2:
        hr, wr = (case.ho + 1) // 2, (case.wo + 1) // 2
        ops["res"] = (torch.randn((n, hr * wr * case.cout), generator=gr) * amp).view(n, hr, wr, case.cout)
    return ops


VARIANTS = ("no_residual", "up2_floor", "drop_last_tap", "drop_last_group", "pad_off_by_one", "roll_scale_bias", "row_shift")


def variants_of(case: Case) -> List[str]:
    v = ["drop_last_group", "pad_off_by_one", "roll_scale_bias", "row_shift"]
    if case.res != RES_NONE:
        v.append("no_residual")
    if case.res == RES_UP2:
        v.append("up2_floor")
    if case.k > 1:
        v.append("drop_last_tap")
    return v


def reference(case: Case, ops: Dict[str, torch.Tensor], variant: Optional[str] = None) -> torch.Tensor:
    """float64 ``act(conv(x, w) * scale + bias + residual)`` of the true f32 operands, as rows [M, Cout] in the kernel's row
    order (image, output row, output column).  ``variant`` names one deliberate mistake (VARIANTS)."""
    assert variant is None or variant in VARIANTS, variant
    x, wt = ops["x"].double(), ops["wt"].double().clone()
    scale, bias = ops["scale"].double(), ops["bias"].double()
    n, ho, wo = x.shape[0], case.ho, case.wo
    if variant == "drop_last_tap":
        wt[:, :, -1, -1] = 0
    if variant == "drop_last_group":
        wt[:, -32:] = 0
    if variant == "roll_scale_bias":
        scale, bias = scale.roll(1), bias.roll(1)
    if case.k == 1 and case.stride == 1 and case.pad == 0 and variant != "pad_off_by_one":
        y = x.reshape(-1, case.cin) @ wt.reshape(case.cout, case.cin).T
    else:
        pad = case.pad + (1 if variant == "pad_off_by_one" else 0)
        y = F.conv2d(x.permute(0, 3, 1, 2), wt, None, stride=case.stride, padding=pad)[:, :, :ho, :wo]
        y = y.permute(0, 2, 3, 1).reshape(-1, case.cout)
    y = y * scale + bias
    if case.res != RES_NONE and variant != "no_residual":
        r = ops["res"].double()
        if case.res == RES_UP2:
            hr, wr = r.shape[1], r.shape[2]
            i, j = torch.arange(ho) // 2, torch.arange(wo) // 2
            if variant == "up2_floor":            # the residual's row pitch and image pitch from floor(Ho / 2), floor(Wo / 2)
                hf, wf = ho // 2, wo // 2
                idx = ((torch.arange(n).view(n, 1, 1) * hf + i.view(1, ho, 1)) * wf + j.view(1, 1, wo)).clamp(max=n * hr * wr - 1)
                r = r.reshape(-1, case.cout)[idx.reshape(-1)]
            else:
                r = r[:, i][:, :, j]
        y = y + r.reshape(-1, case.cout)
    if case.relu:
        y = y.clamp(min=0)
    if variant == "row_shift":
        y = y.roll(1, 0)
    return y


def normalised_error(got: torch.Tensor, ref: torch.Tensor) -> float:
    return float((got.double() - ref).abs().max() / ref.abs().max())


# rows per image of the scale-group tests: 8 x 16 = 128 (the documented minimum) and 12 x 12 = 144
GROUP_GEOS = [("8x16k1", 8, 16, 1, 0), ("12x12k3", 12, 12, 3, 1)]
GROUP_AMPS = (1.0, 100.0, 1.0, 0.01, 1.0)       # neighbouring images 100x apart
