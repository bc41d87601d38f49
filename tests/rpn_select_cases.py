"""The named cases RPN proposal selection is tested on (``test_cpu_rpn_select_ref.py``, ``test_gpu_rpn_select_edges.py``):
tiny five-level pyramids, two or three images of different content each, and in every case the reason it exists -- the
branch of ``csrc/proposals.hip`` (``rpn_level_kernel``, ``rpn_merge_kernel``) or the rule of the contract it is there for.

Every case is built from seeds and literals here, eagerly and deterministically.  The seeds are CHOSEN: apart from the
cases marked ``exact`` the reference's own decisions (``rpn_select_ref.proposals``) keep a distance from every threshold
(``MIN_IOU_MARGIN``, ``MIN_PX_MARGIN``), so that float32 against float64 rounding cannot change a kept set; the CPU test
asserts it for every case.  The ``exact`` cases sit ON the NMS threshold with integer coordinates, areas and
intersections: their quotient is exactly 0.5 or 0.75 in float32 and float64 alike.
"""
from dataclasses import dataclass, field

import numpy as np

import rpn_select_ref as REF

f32 = np.float32

MIN_IOU_MARGIN = 1e-4        # smallest |IoU - thresh| over every pair a greedy pass tested (cases not marked exact)
MIN_PX_MARGIN = 1e-3         # smallest positive clipped extent / emptiness-deciding distance, pixels

# Largest |float32 decode - float64 decode| of a coordinate over every output row of this table, in units of 2^-24 S with
# S = |centre| + |d size| + exp(dsize) size of that axis (``rpn_select_ref.decode_f32`` against ``decode``, clipped).
# Measured and guarded by test_cpu_rpn_select_ref.py (it prints the figure and fails when it leaves this record); the GPU
# bar is 4 x this: device expf may differ from numpy's by an ulp or two, a wrong anchor, stride or delta column shows at
# whole pixels.  Measured: 8.152, at nms_dense_clusters (image 2, row 3, y1): centre deltas of about 10 anchor heights multiply
# the float32 rounding of the anchor's own corners (|shift + cell| near 80 px against a height of 5.7 px).
F32_VS_REF = 8.2

SHAPES = ((24, 20), (15, 10), (6, 5), (3, 3), (1, 1))       # 1440, 450, 90, 27 and 3 logits
STRIDES = (4, 8, 16, 32, 64)
IMG_H, IMG_W = 95, 78                                       # not multiples of any stride
SIZES = (8, 16, 32, 64, 128)
RATIOS = (0.5, 1.0, 2.0)
NAN = np.uint32(0x7FC00000).view(f32)                        # the positive-sign quiet NaN
CLAMP32 = f32(REF.SCALE_CLAMP)


def cell_table(sizes=SIZES) -> np.ndarray:
    """[5, 3, 4] float32: the generator's (x1, y1, x2, y2) of the three aspect ratios at the origin, per level."""
    out = np.zeros((5, 3, 4), dtype=f32)
    for lv, s in enumerate(sizes):
        for a, r in enumerate(RATIOS):
            w = (s * s / r) ** 0.5
            h = r * w
            out[lv, a] = (-w / 2, -h / 2, w / 2, h / 2)
    return out


def square_cells(half) -> np.ndarray:
    """[5, 3, 4]: three squares of half-sides ``half[0..2]`` on every level."""
    out = np.zeros((5, 3, 4), dtype=f32)
    for a, h in enumerate(half):
        out[:, a] = (-h, -h, h, h)
    return out


@dataclass
class Case:
    name: str
    why: str
    heads: list                         # five float32 arrays [N, H, W, head_ld]
    cell: np.ndarray = field(default_factory=cell_table)
    strides: tuple = STRIDES
    img_h: int = IMG_H
    img_w: int = IMG_W
    pre_topk: int = 1000
    post_topk: int = 1000
    nms_thresh: float = 0.7
    base_offset: int = 0                # floats by which the device copy of every head is shifted off its 16-byte alignment
    exact: bool = False                 # a decision ON the NMS threshold, exact in float32 and float64 (no margin asked)
    expect: dict = field(default_factory=dict)   # what the reference must say, per image: checked by the CPU test

    @property
    def head_ld(self) -> int:
        return self.heads[0].shape[3]

    @property
    def n_images(self) -> int:
        return self.heads[0].shape[0]


def random_heads(seed, n=2, shapes=SHAPES, ld=16, delta_scale=0.3, junk=True):
    """randn logits, randn * delta_scale deltas; columns from 15 on are LARGE finite junk of both signs (never data)."""
    rng = np.random.default_rng(seed)
    heads = []
    for (h, w) in shapes:
        x = rng.standard_normal((n, h, w, ld)).astype(f32)
        x[..., 3:15] *= f32(delta_scale)
        if ld > 15:
            x[..., 15:] = (f32(3e37) if junk else f32(0)) * np.sign(x[..., 15:])
        heads.append(x)
    return heads


def quiet_heads(n, shapes=SHAPES, ld=16, seed=0):
    """Zero deltas and distinct, very low logits (-20 .. -10, descending with a seeded shuffle): a background that decodes to
    the anchors themselves and never outranks a planted row."""
    rng = np.random.default_rng(seed)
    heads = []
    for (h, w) in shapes:
        x = np.zeros((n, h, w, ld), dtype=f32)
        for i in range(n):
            x[i, :, :, :3] = (-10.0 - 10.0 * rng.permutation(h * w * 3) / (h * w * 3)).astype(f32).reshape(h, w, 3)
        heads.append(x)
    return heads


def plant(heads, n, lv, h, w, a, logit, deltas=None):
    heads[lv][n, h, w, a] = f32(logit)
    if deltas is not None:
        heads[lv][n, h, w, 3 + 4 * a:7 + 4 * a] = np.asarray(deltas, dtype=f32)


def _ref(case: Case):
    return REF.proposals(case.heads, case.cell, case.strides, case.img_h, case.img_w, case.pre_topk, case.post_topk, case.nms_thresh)


# ---- selection ---------------------------------------------------------------------------------------------------------
def _selection_cases():
    cases = [Case("select_smooth", "random logits: a level of 1440 (> pre_topk: histogram select + candidate list) and levels of 450, 90, "
                  "27 and 3 (< pre_topk: everything selected, k = total)", random_heads(101, n=3))]
    hd = random_heads(1, n=2)
    for x in hd:
        x[..., :3] = np.round(x[..., :3] * 4) / 4 + f32(0.0)             # (+ 0.0: a -0.0 from rounding becomes +0.0, see rpn_select_ref)
    cases.append(Case("select_quantised", "logits on a grid of 1/4: about 25 distinct values, hundreds of equal logits straddle the cut of "
                      "level 0 (lowest index first), and ties within and across levels in the merge", hd))
    hd = random_heads(4, n=2)
    hd[0][..., :3] = f32(-2.5)
    hd[2][1, ..., :3] = f32(0.75)
    cases.append(Case("select_all_equal", "level 0 all -2.5 (the first 1000 indices are the selection) and, in image 1, level 2 all 0.75", hd))
    shapes = ((56, 56),) + SHAPES[1:]
    hd = random_heads(1, n=2, shapes=shapes)
    hd[0][..., :3] = f32(1.0) + hd[0][..., :3] * f32(1e-3)
    cases.append(Case("select_two_bins", "9408 logits of level 0 around 1.0: two 12-bit key bins either side of a power of two, the upper one holds "
                      "the cut and about 4700 candidates (no overflow)", hd, img_h=222, img_w=219))
    hd = random_heads(0, n=2, shapes=shapes)
    hd[0][..., :3] = f32(1.0625) + hd[0][..., :3] * f32(1e-3)
    cases.append(Case("select_overflow", "9408 logits of level 0 all in [1, 1.125) = ONE 12-bit key bin: the candidate list (8192) "
                      "overflows and the radix passes run", hd, img_h=222, img_w=219))
    shapes = ((52, 52),) + SHAPES[1:]
    hd = random_heads(2, n=2, shapes=shapes)
    hd[0][..., :3] = f32(1.0625) + hd[0][..., :3] * f32(1e-3)
    cases.append(Case("select_one_bin_fits", "8112 logits in one 12-bit bin: the candidate list is filled to 8112 of 8192 and sorted whole",
                      hd, img_h=206, img_w=203))
    # signs and extremes: level 0 takes 1000 of 1440, level 1 takes all 450
    hd = random_heads(0, n=2)
    for n in range(2):
        rng = np.random.default_rng(50 + n)
        lg = hd[0][n, :, :, :3].reshape(-1).copy()
        lg = -np.abs(lg) - f32(0.01)                                   # all negative, distinct: the cut falls among these
        p = rng.permutation(1440)
        lg[p[:3]] = NAN
        lg[p[3:7]] = f32(np.inf)
        lg[p[7:200]] = np.abs(lg[p[7:200]])                            # positive
        z = np.sort(p[200:300])
        lg[z[:50]] = f32(0.0)                                          # every +0.0 at a lower index than every -0.0
        lg[z[50:]] = f32(-0.0)
        lg[p[300:320]] = f32(-np.inf)                                  # 1420 logits lie above: never selected
        hd[0][n, :, :, :3] = lg.reshape(24, 20, 3)
        l1 = hd[1][n, :, :, :3].reshape(-1).copy()
        q = rng.permutation(450)
        l1[q[:2]] = NAN
        l1[q[2:4]] = f32(np.inf)
        l1[q[4:9]] = f32(-np.inf)                                      # selected (k = total), dropped: not finite
        hd[1][n, :, :, :3] = l1.reshape(15, 10, 3)
    cases.append(Case("select_signs_and_extremes", "negative logits at the cut; +0.0 / -0.0 (tied or not: the same order either way, see "
                      "rpn_select_ref), +inf and positive NaN on top (selected, then dropped), -inf at the bottom", hd))
    return cases


def _topk_cases():
    cases = []
    for k, seed in ((1, 0), (63, 0), (64, 0), (65, 0), (1000, 0)):
        cases.append(Case(f"pre_topk_{k}", f"pre_topk = {k}: " + {1: "one row per level", 63: "one short of a 64-candidate word", 64: "exactly one word",
                          65: "one row in the second word", 1000: "the production value"}[k], random_heads(200 + 10 * k + seed, n=2), pre_topk=k))
    base = Case("post_topk_1", "post_topk = 1: the best survivor of the five levels only", random_heads(300, n=2), post_topk=1)
    cases.append(base)
    hd = random_heads(301, n=2)
    full = Case("", "", hd, pre_topk=150)
    least = min(r["survivors"] for r in _ref(full))
    cases.append(Case("post_topk_one_below_survivors", f"post_topk = {least - 1}: one below the smaller image's survivor count (pre_topk = 150), the last survivor is cut",
                      hd, pre_topk=150, post_topk=least - 1, expect=dict(min_survivors=least)))
    cases.append(Case("post_topk_1000_few_survivors", "pre_topk = 64: at most 64 + 64 + 64 + 27 + 3 survivors in 1000 output rows, the tail exactly zero",
                      random_heads(302, n=3), pre_topk=64))
    cases.append(Case("post_topk_1024", "the largest post_topk the library takes", random_heads(304, n=2), post_topk=1024))
    return cases


def _head_ld_cases():
    return [
        Case("head_ld_15", "rows of 15 floats, no padding: scalar loads", random_heads(400, n=2, ld=15)),
        Case("head_ld_17", "rows of 17 floats (junk in column 15 and 16): scalar loads, every row at another alignment", random_heads(401, n=3, ld=17)),
        Case("head_ld_20", "rows of 20 floats, 16-byte aligned: vector loads beside five junk columns", random_heads(404, n=2, ld=20)),
        Case("head_ld_16_base_offset_1", "rows of 16 floats on a base shifted by one float: misaligned, scalar loads", random_heads(403, n=2), base_offset=1),
    ]


# ---- decode edges ------------------------------------------------------------------------------------------------------
# 2 x 2 px anchors (cells +-1) on a stride of 16 / 32 / ..: the background boxes are disjoint, a clamped size delta gives
# 125 px (62.5 x 2), well inside the 381 x 317 image -- so the clamp's VALUE is in the output, not hidden by clipping
DEC_STRIDES = (16, 32, 64, 128, 256)
DEC_H, DEC_W = 381, 317
DEC_SHAPES = ((24, 20), (12, 10), (6, 5), (3, 3), (1, 1))


def _dec_case(name, why, n, planter, **kw):
    hd = quiet_heads(n, shapes=DEC_SHAPES, ld=16, seed=len(name))
    planter(hd)
    return Case(name, why, hd, cell=square_cells((1.0, 1.0, 1.0)), strides=DEC_STRIDES, img_h=DEC_H, img_w=DEC_W, **kw)


def _decode_cases():
    below = np.nextafter(CLAMP32, f32(0))

    def clamp(hd):
        # image 0: width deltas, one row each on rows h = 2, 6, 10, 14, 18 at w = 9 (centre x = 144: +-62.5 is inside);
        # image 1: height deltas on columns w = 2, 6, 10, 14, 18 at h = 11 (centre y = 176)
        for i, v in enumerate((CLAMP32, below, f32(10.0), f32(100.0), f32(np.inf))):
            plant(hd, 0, 0, 2 + 4 * i, 9, i % 3, 5.0 - i, (0.25, -0.5, v, 0.5))
            plant(hd, 1, 0, 11, 2 + 4 * i, (i + 1) % 3, 5.0 - i, (-0.5, 0.25, 0.5, v))
        # image 2: both at once on level 1 (stride 32), plus a delta of 4.0 (just under: 54.6 x) that must NOT be clamped
        plant(hd, 2, 1, 5, 4, 0, 5.0, (0.0, 0.0, f32(100.0), f32(np.inf)))
        plant(hd, 2, 0, 3, 3, 1, 4.0, (0.0, 0.0, f32(4.0), f32(4.0)))
    cases = [_dec_case("decode_size_clamp", "size deltas at, one float under, above (10), far above (100, unclamped exp overflows float32) and +inf: "
                       "clamped to log(1000 / 16), finite, 125 px, kept", 3, clamp)]

    def not_finite(hd):
        # every planted row outranks the background; what must be dropped would otherwise lead the output
        for n, v in enumerate((NAN, f32(np.inf), f32(-np.inf))):
            for slot in range(4):
                d = [0.25, 0.25, 0.5, 0.5]
                d[slot] = v
                plant(hd, n, 0, 3 + 4 * slot, 5 + 2 * slot, slot % 3, 9.0 - slot, d)
                d2 = [0.0, 0.0, 0.0, 0.0]
                d2[slot] = v
                plant(hd, n, 2, slot, slot, (slot + 1) % 3, 8.5 - slot, d2)
            plant(hd, n, 0, 20, 3, 0, 3.0, (0.5, 0.5, 1.0, 1.0))        # an ordinary row after them
    cases.append(_dec_case("decode_not_finite_deltas", "NaN (image 0), +inf (image 1), -inf (image 2) in each of the four delta slots of "
                           "top-ranked rows: NaN anywhere and +-inf centre deltas drop the row, a +inf size delta is clamped and kept, a -inf size "
                           "delta gives extent 0 and is dropped as empty", 3, not_finite))

    def outside(hd):
        # anchor (h, w) has its centre at (16 w, 16 h), 2 px wide; d * 2 px shifts it
        plant(hd, 0, 0, 5, 0, 0, 9.0, (-100.0, 0.0, 1.0, 1.0))          # wholly left of 0
        plant(hd, 0, 0, 5, 19, 1, 8.0, (100.0, 0.0, 1.0, 1.0))          # wholly right of img_w
        plant(hd, 0, 0, 0, 5, 2, 7.0, (0.0, -100.0, 1.0, 1.0))          # above
        plant(hd, 0, 0, 23, 5, 0, 6.0, (0.0, 100.0, 1.0, 1.0))          # below
        plant(hd, 0, 0, 0, 0, 1, 5.0, (-100.0, -100.0, 1.0, 1.0))       # outside a corner
        # image 1: x2 = +-2^-9 before clipping (anchor at w = 0: x = -1 .. 1, shifted by d * 2): kept with width 2^-9 / dropped
        e = 2.0 ** -9
        plant(hd, 1, 0, 4, 0, 0, 9.0, ((-1 + e) / 2, 0.0, 0.0, 0.0))
        plant(hd, 1, 0, 8, 0, 1, 8.0, ((-1 - e) / 2, 0.0, 0.0, 0.0))
        plant(hd, 1, 0, 0, 4, 2, 7.0, (0.0, (-1 + e) / 2, 0.0, 0.0))    # the same for y2
        plant(hd, 1, 0, 0, 8, 0, 6.0, (0.0, (-1 - e) / 2, 0.0, 0.0))
        # x1 = img_w -+ 2^-9 (anchor at w = 19: x = 303 .. 305; img_w = 317 -> shift by 14 -+ e): kept / dropped; and y1 at img_h
        plant(hd, 1, 0, 12, 19, 1, 5.0, ((14 - e) / 2, 0.0, 0.0, 0.0))
        plant(hd, 1, 0, 16, 19, 2, 4.0, ((14 + e) / 2, 0.0, 0.0, 0.0))
        plant(hd, 1, 0, 23, 12, 0, 3.0, (0.0, (14 - e) / 2, 0.0, 0.0))   # h = 23: y = 367 .. 369; img_h = 381
        plant(hd, 1, 0, 23, 16, 1, 2.0, (0.0, (14 + e) / 2, 0.0, 0.0))
        # image 2: width exactly 0 ON the border (size delta -inf: extent 0 before clipping as well) and straddling boxes
        plant(hd, 2, 0, 6, 0, 0, 9.0, (0.0, 0.0, f32(-np.inf), 0.0))    # x1 = x2 = 0
        plant(hd, 2, 0, 0, 6, 1, 8.0, (0.0, 0.0, 0.0, f32(-np.inf)))    # y1 = y2 = 0
        plant(hd, 2, 0, 10, 0, 2, 7.0, (0.0, 0.0, 3.0, 0.0))            # straddles the left border: clipped, kept
        plant(hd, 2, 0, 23, 19, 0, 6.0, (2.0, 2.0, 3.0, 3.0))           # straddles the bottom right corner
    cases.append(_dec_case("decode_outside_and_borders", "boxes wholly outside on each side and a corner (empty after clipping only); x2 / y2 at "
                           "+-2^-9 and x1 / y1 at the far border -+2^-9 (kept / dropped); extent exactly 0 on the border; an image of 381 x 317 "
                           "on strides of 16", 3, outside))
    return cases


# ---- NMS ---------------------------------------------------------------------------------------------------------------
def _nms_cases():
    cases = []
    # dense: 1000 selected anchors of level 0 pushed into clusters of 16 x 16 boxes jittered by +-0.4 px (IoU within a cluster
    # >= (15.2 / 16.8)^2 = 0.82, between clusters 0); the remaining 440 anchors rank below them
    hd = random_heads(500, n=3)
    cell = cell_table()
    centres = ((18.0, 18.0), (58.0, 18.0), (18.0, 58.0), (58.0, 58.0), (38.0, 80.0))
    for n in range(3):
        rng = np.random.default_rng(510 + n)
        perm = rng.permutation(1440)                                    # rank r <- flattened index perm[r]
        lg = np.empty(1440, dtype=f32)
        lg[perm] = (4.0 - 8.0 * np.arange(1440) / 1440).astype(f32)     # distinct, descending with the rank
        hd[0][n, :, :, :3] = lg.reshape(24, 20, 3)
        late = (0, 200, 700)[n]                                         # cluster 4 appears from this rank on only: its survivor sits in word late // 64
        for r in range(1000):
            i = int(perm[r])
            a, loc = i % 3, i // 3
            h, w = loc // 20, loc % 20
            c = int(rng.integers(0, 5 if r >= late else 4))
            if r == late:
                c = 4
            tx, ty = centres[c][0] + rng.uniform(-0.4, 0.4), centres[c][1] + rng.uniform(-0.4, 0.4)
            aw, ah = float(cell[0, a, 2] - cell[0, a, 0]), float(cell[0, a, 3] - cell[0, a, 1])
            hd[0][n, h, w, 3 + 4 * a:7 + 4 * a] = ((tx - 4.0 * w) / aw, (ty - 4.0 * h) / ah, np.log(16.0 / aw), np.log(16.0 / ah))
    cases.append(Case("nms_dense_clusters", "the 1000 selected rows of level 0 in five tight clusters: each keeps its first member, whose row is "
                      "OR-ed into every later 64-candidate word (word 0 into 1 .. 15; the fifth cluster's survivor sits in word 0, 3 and 10)",
                      hd, expect=dict(level0_survivors=5)))

    # chains on disjoint 2 x 2 background boxes: 20 x 20 boxes shifted by 4 px (IoU 16 / 24) and 8 px (12 / 28), thresh 0.5
    def chains(hd):
        ranks = {0: ((62, 63, 64), (10, 11, 12)), 1: ((63, 64, 66), (126, 128, 129)), 2: ((62, 65, 66), (127, 128, 130))}
        for n, cs in ranks.items():
            for ci, (ra, rb, rc) in enumerate(cs):
                for j, r in enumerate((ra, rb, rc)):
                    # rank r: logit 9 - r / 100; the planted rows fill every rank up to the last chain's, the others are singles
                    plant(hd, n, 0, 6 + 10 * ci, 10 + j, j, 9.0 - r / 100.0, (2.0 * j - 8.0 * j, 0.0, np.log(10.0), np.log(10.0)))
            used = {r for c in cs for r in c}
            free = [(h, w) for h in range(24) for w in range(20) if h not in (6, 16, 5, 7, 15, 17)]
            k = 0
            for r in range(0, 131):
                if r in used:
                    continue
                h, w = free[k]
                k += 1
                plant(hd, n, 0, h, w, r % 3, 9.0 - r / 100.0, (0.0, 0.0, 0.0, 0.0))
    cases.append(_dec_case("nms_chain_across_words", "chains A > B > C (A suppresses B, B would suppress C, A does not: C survives) at ranks "
                           "62-63-64, 63-64-66 and 62-65-66 (one image each) across the first word boundary, and at 10-11-12, 126-128-129, 127-128-130",
                           3, chains, nms_thresh=0.5, expect=dict(chains=True)))

    def invalid(hd):
        # rank 0 has a +inf score (image 0) / NaN score (image 1) / NaN dy (image 2) and a box that would suppress rank 1 (IoU 0.82)
        for n, (lg, d) in enumerate(((np.inf, (0.0, 0.0, 2.0, 2.0)), (NAN, (0.0, 0.0, 2.0, 2.0)), (9.0, (0.0, NAN, 2.0, 2.0)))):
            plant(hd, n, 0, 8, 8, 0, lg, d)
            plant(hd, n, 0, 8, 9, 1, 8.0, (-7.5, 0.25, 2.0, 2.0))      # centre 144 - 15 = 129 against 128: 14.78 px boxes one pixel apart
            plant(hd, n, 0, 8, 10, 2, 7.0, (-15.0, 0.0, 2.0, 2.0))      # and a third that rank 1 DOES suppress
    cases.append(_dec_case("nms_invalid_row_suppresses_nothing", "the top row is invalid (+inf score, NaN score, NaN delta) and lies on rank 1: "
                           "rank 1 survives and suppresses rank 2", 3, invalid))
    return cases


def _threshold_cases():
    """Anchor 0: +-24 squares, neighbours two cells (16 px) apart: IoU = 32 * 48 / (2 * 2304 - 1536) = 1 / 2.
    Anchor 1: +-28 squares, neighbours one cell (8 px) apart: IoU = 48 * 56 / (2 * 3136 - 2688) = 3 / 4.
    pre_topk = 2: the pair is the whole selection of its level.  Centre deltas are exact binary fractions, size deltas zero."""
    cases = []
    shapes = ((12, 10), (12, 10), (6, 5), (3, 3), (1, 1))
    cell = square_cells((24.0, 28.0, 2.0))
    for value, a, step in ((0.5, 0, 2), (0.75, 1, 1)):
        for which, thr in (("at", f32(value)), ("below", np.nextafter(f32(value), f32(0)))):
            hd = quiet_heads(2, shapes=shapes, seed=7)
            for n in range(2):
                for lv in (0, 1):
                    h = 5 + n
                    dy = (0.125, -0.25)[lv]                             # the same shift for both boxes: 6 (7) px down, 12 (14) px up
                    plant(hd, n, lv, h, 4, a, 3.0 - lv, (0.0, dy, 0.0, 0.0))
                    plant(hd, n, lv, h, 4 + step, a, 2.0 - lv, (0.0, dy, 0.0, 0.0))
            cases.append(Case(f"nms_thresh_exactly_{value}_{which}", f"a pair with IoU exactly {value}, nms_thresh "
                              + ("equal to it: not suppressed (strict >)" if which == "at" else "one float below it: suppressed"),
                              hd, cell=cell, strides=(8, 8, 16, 32, 64), img_h=96, img_w=80, pre_topk=2, nms_thresh=float(thr), exact=True,
                              expect=dict(rows_of_levels_0_1=4 if which == "at" else 2)))
    return cases


def _level_and_merge_cases():
    cases = []
    hd = quiet_heads(2, seed=3)
    cell = square_cells((12.0, 6.0, 3.0))
    for n in range(2):
        plant(hd, n, 0, 4 + 2 * n, 4, 0, 3.0, (0.0, 0.0, 0.0, 0.0))     # level 0, stride 8: centre (32, 32 + 16 n)
        plant(hd, n, 1, 2 + n, 2, 0, 2.0, (0.0, 0.0, 0.0, 0.0))         # level 1, stride 16: the same box
        plant(hd, n, 0, 4 + 2 * n, 5, 0, 1.0, (-0.25, 0.0, 0.0, 0.0))   # and, on level 0, a third that the first suppresses (IoU 22 / 26)
    cases.append(Case("levels_do_not_interact", "identical boxes (IoU 1) on level 0 and level 1: both survive; a third on level 0 does not",
                      hd, cell=cell, strides=(8, 16, 32, 64, 128), img_h=190, img_w=158, expect=dict(top=[(0, 3.0), (1, 2.0)])))
    hd = quiet_heads(3, seed=4)
    cell = square_cells((1.0, 1.0, 1.0))
    for n in range(3):
        # equal scores across levels, planted in an order that is NOT the level order, and equal scores within a level
        for lv in ((3, 0, 2, 1, 4), (4, 2, 0, 3, 1), (1, 4, 3, 0, 2))[n]:
            at = (5, 3, 2, 1, 0)[lv]                                        # another place on every level: five different boxes
            plant(hd, n, lv, at, at, (lv + n) % 3, 2.0)
        plant(hd, n, 0, 7, 3, 2, 1.5)
        plant(hd, n, 0, 2, 11, 0, 1.5)
        plant(hd, n, 0, 2, 3, 1, 1.5)
        plant(hd, n, 1, 1, 1, 1, 1.5)
        plant(hd, n, 2, 3, 2, 0, 1.75)                                  # between the two tie groups, on a later level
    cases.append(Case("merge_ties", "a score of 2.0 on every level (lower level first), 1.75 on level 2, then 1.5 three times on level 0 "
                      "(lower rank = lower index first) and once on level 1", hd, cell=cell, strides=DEC_STRIDES, img_h=DEC_H, img_w=DEC_W,
                      expect=dict(lead=[(0, 2.0), (1, 2.0), (2, 2.0), (3, 2.0), (4, 2.0), (2, 1.75), (0, 1.5), (0, 1.5), (0, 1.5), (1, 1.5)])))
    # zero survivors in image 0, by a different reason on every level; image 1 is an ordinary random image
    hd = random_heads(600, n=2)
    hd[0][0, ..., 3:15:4] = NAN                                         # dx
    hd[1][0, ..., 3:15:4] = f32(-1000.0)                                # wholly left of the image
    hd[2][0, ..., :3] = f32(np.inf)                                     # scores
    hd[3][0, ..., 5:15:4] = f32(-np.inf)                                # dw: extent 0
    hd[4][0, ..., 4:15:4] = f32(np.inf)                                 # dy
    cases.append(Case("zero_survivors", "every selected row of image 0 is invalid (NaN dx, outside, +inf score, -inf dw, +inf dy by level): "
                      "count 0 and zero rows, image 1 beside it unaffected", hd, expect=dict(count0=0)))
    return cases


def _random_cases():
    return [Case(f"random_{i}", "seeded random heads, deltas x 0.3, production parameters", random_heads(seed, n=3)) for i, seed in enumerate((700, 706, 711))]


CASES = (_selection_cases() + _topk_cases() + _head_ld_cases() + _decode_cases() + _nms_cases() + _threshold_cases()
         + _level_and_merge_cases() + _random_cases())
NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

_REFS = {}


def reference(case: Case) -> list:
    """The reference's result for every image of ``case``: computed once, shared, read only."""
    if case.name not in _REFS:
        res = _ref(case)
        for r in res:
            for k in ("boxes", "scores", "src", "S"):
                r[k].setflags(write=False)
        _REFS[case.name] = res
    return _REFS[case.name]
