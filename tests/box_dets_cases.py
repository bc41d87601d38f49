"""The named cases box detection selection is tested on (``test_cpu_box_dets_ref.py``, ``test_gpu_box_dets_edges.py``):
tiny batches of two to five images with different content and different ``prop_count``, and in every case the reason it
exists -- the branch of ``box_detections_kernel`` (``csrc/proposals.hip``) or the rule of the contract it is there for.

Every case is built from seeds and literals here, eagerly and deterministically.  The seeds are CHOSEN: apart from the
cases marked ``exact`` the reference's own decisions (``box_dets_ref.detections``) keep a distance from every threshold, so
that float32 against float64 rounding cannot change a kept set or its order; the CPU test asserts it for every case:
  * |score - thresh| and the gap between two candidates' scores that do not tie: at least 16 x ``F32_VS_REF_SCORE`` x 2^-24;
  * candidates that tie do so bit for bit, in float64 and in the float32 restatement alike (bit-identical logit rows, or
    equal class logits in one row);
  * every pair the greedy pass tests decides alike in float64, in plain float32 and in shifted float32, with
    |IoU - thresh| at least ``MIN_IOU_MARGIN`` and at least 16 x that pair's own |IoU_f32 - IoU_f64|;
  * a finite-test decision lies at least ``MIN_FINITE_MARGIN`` binades from the float32 overflow threshold.
The ``exact`` cases sit ON a threshold with values that are exact in float32 and float64 alike: equal logits (a score of
exactly 1 / 2 or 1 / 4), integer coordinates (an IoU of exactly 1 / 2).  Pairs that sit on the NMS threshold only under
float32 rounding stay with ``test_box_detections_follow_torchvisions_batched_nms_branch_on_threshold_pairs``.
"""
import math
from dataclasses import dataclass, field

import numpy as np

import box_dets_ref as REF

f32 = np.float32

MIN_IOU_MARGIN = 1e-4        # smallest |IoU - thresh| over every pair a greedy pass tested (the RPN table's value)
MIN_FINITE_MARGIN = 0.5      # binades between a value the finite test hangs on and the float32 overflow threshold

# Largest |float32 restatement - reference| over every kept row of this table (``box_dets_ref.dets_f32`` against
# ``detections``): scores in units of 2^-24, box coordinates in units of 2^-24 S with S = |centre| + |d size| +
# exp(dsize) size of that axis.  Measured and guarded by test_cpu_box_dets_ref.py (it prints both figures and fails when
# they leave these records); the GPU bars are 4 x these: device expf may differ from numpy's by an ulp or two, while a
# wrong column, weight or class shows at whole pixels or whole classes.
# Measured: score 2.465 at ld_exact_odd_K (image 1, output row 0): a score of 0.954, where 2^-24 is the float32 spacing
#           itself: four exp, a four-term sum and a quotient, each rounded once;
#           box 2.216 at random_0 (image 2, output row 1, x2 = 153.2 with S = 167.0): the centre, the size delta over its
#           weight, exp, two products and the sum, each rounded once at the scale of S.
F32_VS_REF_SCORE = 2.5
F32_VS_REF_BOX = 2.3
F32_VS_REF_SCORE_AT = ("ld_exact_odd_K", 1, 0)                # (case, image, output row)
F32_VS_REF_BOX_AT = ("random_0", 2, 1, 2)                     # (case, image, output row, coordinate)

IMG_H, IMG_W = 300, 420                                       # not square
THRESH = 0.05
QUIET = 1e-6                                                  # the score of a class nobody asks for
NAN = np.uint32(0x7FC00000).view(f32)
CLAMP = REF.SCALE_CLAMP


@dataclass
class Case:
    name: str
    why: str
    logits: np.ndarray                  # [N, R, ld] float32
    props: np.ndarray                   # [N, R, 4] float32
    prop_count: np.ndarray              # [N] int32
    K: int
    img_h: int = IMG_H
    img_w: int = IMG_W
    score_thresh: float = THRESH
    nms_thresh: float = 0.5
    topk: int = 100
    exact: bool = False                 # a decision ON a threshold, exact in float32 and float64 (no margin asked)
    expect: dict = field(default_factory=dict)

    @property
    def n_images(self) -> int:
        return self.logits.shape[0]

    @property
    def R(self) -> int:
        return self.logits.shape[1]

    @property
    def ld(self) -> int:
        return self.logits.shape[2]


# ---- building blocks -----------------------------------------------------------------------------------------------------
def grid_props(n, r, size=8.0, pitch=12, cols=8, at=(2.0, 2.0)) -> np.ndarray:
    """[n, r, 4]: disjoint squares of ``size`` on a grid, integer coordinates."""
    i = np.arange(r)
    x, y = at[0] + (i % cols) * pitch, at[1] + (i // cols) * pitch
    one = np.stack([x, y, x + size, y + size], axis=1).astype(f32)
    return np.repeat(one[None], n, axis=0).copy()


def quiet(n, r, k, ld=None, junk=3e37, **grid):
    """Rows nobody asks for: every class at a score of 1e-6, zero deltas, disjoint boxes.  Columns from 5 k + 1 on hold
    LARGE finite junk of both signs (never data)."""
    ld = 5 * k + 1 if ld is None else ld
    lg = np.zeros((n, r, ld), dtype=f32)
    lg[..., :k] = f32(math.log(QUIET))
    if ld > 5 * k + 1:
        sign = np.where((np.arange(n * r * (ld - 5 * k - 1)) % 3) == 0, -1.0, 1.0).reshape(n, r, -1)
        lg[..., 5 * k + 1:] = (junk * sign).astype(f32)
    return lg, grid_props(n, r, **grid), np.full((n,), r, dtype=np.int32)


def set_probs(lg, n, r, k, probs):
    """The class logits of row ``r`` for the target scores ``probs`` {class: score} (the others 1e-6, the background the rest)."""
    p = np.full(k + 1, QUIET)
    for c, v in probs.items():
        p[c] = v
    p[k] = 1.0 - p[:k].sum()
    assert p[k] > 0, (probs, p[k])
    lg[n, r, :k + 1] = np.log(p).astype(f32)


def set_deltas(lg, n, r, k, c, d):
    lg[n, r, k + 1 + 4 * c:k + 5 + 4 * c] = np.asarray(d, dtype=f32)


def plant(lg, pr, n, r, k, probs, deltas=None, prop=None):
    set_probs(lg, n, r, k, probs)
    for c, d in (deltas or {}).items():
        set_deltas(lg, n, r, k, c, d)
    if prop is not None:
        pr[n, r] = np.asarray(prop, dtype=f32)


def counts(*c) -> np.ndarray:
    """prop_count per image: different from image to image; the rows from the count on are rows the case does not use."""
    return np.asarray(c, dtype=np.int32)


def _ref(case: Case):
    return REF.detections(case.logits, case.props, case.prop_count, case.K, case.img_h, case.img_w, case.score_thresh,
                          case.nms_thresh, case.topk)


def random_case(name, why, seed, n, r, k, ld=None, counts=None, **kw) -> Case:
    """randn x 1.5 logits, randn x 0.5 deltas, boxes of 20 .. 40 px jittered by +-3 px around r / 4 centres."""
    rng = np.random.default_rng(seed)
    lg, pr, cnt = quiet(n, r, k, ld)
    lg[..., :k + 1] = (rng.standard_normal((n, r, k + 1)) * 1.5).astype(f32)
    lg[..., k + 1:5 * k + 1] = (rng.standard_normal((n, r, 4 * k)) * 0.5).astype(f32)
    ncl = max(2, r // 4)
    for i in range(n):
        cx, cy = rng.uniform(30, IMG_W - 30, ncl), rng.uniform(30, IMG_H - 30, ncl)
        which = rng.integers(0, ncl, r)
        x, y = cx[which] + rng.uniform(-3, 3, r), cy[which] + rng.uniform(-3, 3, r)
        w, h = rng.uniform(20, 40, r), rng.uniform(20, 40, r)
        pr[i] = np.stack([x - w / 2, y - h / 2, x + w / 2, y + h / 2], axis=1).astype(f32)
    if counts is not None:
        cnt = np.asarray(counts, dtype=np.int32)
    return Case(name, why, lg, pr, cnt, k, **kw)


def dense_case(name, why, seed, r, k, cand, lo, hi, clusters, counts=None, same_deltas=False, img=(IMG_H, IMG_W), **kw) -> Case:
    """``cand`` [n, r, k] bool: the slots that are candidates get evenly spaced, distinct scores in [lo, hi) in a seeded
    order (hi x k < 1); the rows sit in ``clusters[i]`` clusters of 16 x 16 boxes on a pitch of 24, jittered by +-0.3 px,
    with centre deltas of +-0.1 (0.16 px) and size deltas of +-0.1 (2 %): IoU above 0.75 inside a cluster, 0 between."""
    rng = np.random.default_rng(seed)
    cand = np.asarray(cand, dtype=bool)
    n = cand.shape[0]
    assert hi * k < 1 and cand.shape == (n, r, k)
    lg, pr, cnt = quiet(n, r, k, kw.pop("ld", None))
    cols = img[1] // 24 - 1
    for i in range(n):
        m = int(cand[i].sum())
        scores = np.full((r, k), QUIET)
        scores[cand[i]] = (lo + (hi - lo) * rng.permutation(m) / max(m, 1))
        p = np.concatenate([scores, 1.0 - scores.sum(axis=1, keepdims=True)], axis=1)
        assert p.min() > 0
        lg[i, :, :k + 1] = np.log(p).astype(f32)
        d = rng.uniform(-0.1, 0.1, (r, 1 if same_deltas else k, 4))
        lg[i, :, k + 1:5 * k + 1] = np.broadcast_to(d, (r, k, 4)).reshape(r, 4 * k).astype(f32)
        ncl = clusters[i] if isinstance(clusters, (tuple, list)) else clusters
        assert ncl <= cols * (img[0] // 24 - 1), (ncl, cols)
        which = np.arange(r) % ncl if ncl >= r else rng.integers(0, ncl, r)
        x = 8.0 + (which % cols) * 24 + rng.uniform(-0.3, 0.3, r)
        y = 8.0 + (which // cols) * 24 + rng.uniform(-0.3, 0.3, r)
        pr[i] = np.stack([x, y, x + 16, y + 16], axis=1).astype(f32)
    if counts is not None:
        cnt = np.asarray(counts, dtype=np.int32)
    return Case(name, why, lg, pr, cnt, k, img_h=img[0], img_w=img[1], **kw)


def ranked_rows(lg, n, k, scores, ties, seed, rows=None):
    """Fill image ``n`` so that its candidates, in rank order, have the target ``scores`` (descending); ``ties`` is a set of
    ranks that repeat the score of the rank before them BIT FOR BIT (a row of their own with the logits of that rank's
    row, the score in class 0).  Ranks that tie with nobody are packed k to a row.  The rows are dealt in a seeded order, so
    rank and row number are unrelated.  Returns {rank: (row, class)}."""
    rng = np.random.default_rng(seed)
    r = lg.shape[1]
    order = list(rng.permutation(r) if rows is None else rng.permutation(np.asarray(rows)))
    where, loose = {}, []
    group_row = {}
    for rank, s in enumerate(scores):
        if rank in ties or rank + 1 in ties:
            row = int(order.pop())
            if rank in ties:
                lg[n, row, :k + 1] = lg[n, group_row[rank - 1], :k + 1]
            else:
                set_probs(lg, n, row, k, {0: s})
            group_row[rank] = row
            where[rank] = (row, 0)
        else:
            loose.append((rank, s))
    rng.shuffle(loose)
    for i in range(0, len(loose), k):
        row = int(order.pop())
        chunk = loose[i:i + k]
        set_probs(lg, n, row, k, {c: s for c, (_, s) in enumerate(chunk)})
        for c, (rank, _) in enumerate(chunk):
            where[rank] = (row, c)
    return where


# ---- rows and strides ----------------------------------------------------------------------------------------------------
def _row_cases():
    cases = [random_case("rows_prop_count_edges", "prop_count = 0, 1, R - 1, R and R + 5 (clamped to R) in one batch: "
                         "R = min(prop_count[n], R) and the per-image offsets n R ld, n R and n topk", 1000, 5, 16, 2, counts=(0, 1, 15, 16, 21))]
    c = random_case("rows_past_count_hold_nan_and_best_scores", "rows from prop_count on hold NaN logits, NaN boxes and, every other row, the "
                    "largest score of the image on a box of its own: none of them may be read", 1001, 3, 24, 2, counts=(5, 12, 22))
    for n, cnt in enumerate(c.prop_count):
        for r in range(int(cnt), 24):
            if (r + n) % 2 == 0:
                c.logits[n, r], c.props[n, r] = NAN, NAN
            else:
                plant(c.logits, c.props, n, r, 2, {0: 0.9999 - 1e-5 * r}, prop=(300 + 4 * r, 10, 330 + 4 * r, 40 + 9 * (r % 2)))
    cases.append(c)
    cases.append(random_case("ld_exact_odd_K", "ld = 5 K + 1 = 16 exactly, K = 3: no pad column", 1002, 3, 20, 3, counts=(20, 13, 7)))
    cases.append(random_case("ld_exact_even_K", "ld = 5 K + 1 = 11 exactly, K = 2: every row at another alignment", 1003, 3, 20, 2, counts=(9, 20, 14)))
    cases.append(random_case("ld_padded_garbage", "ld = 16 for K = 2: columns 11 .. 15 hold +-3e37 and are never data", 1004, 2, 20, 2, ld=16, counts=(20, 11)))
    for k, r, seed in ((1, 40, 1010), (2, 40, 1011), (3, 40, 1012), (5, 24, 1020), (8, 24, 1014)):
        cases.append(random_case(f"classes_K{k}", f"K = {k}: the softmax over {k + 1} columns, deltas from column {k + 1}, "
                                 f"candidate id = row x {k} + class" + (", ld = 44 with three junk columns" if k == 8 else ""),
                                 seed, 2, r, k, ld=44 if k == 8 else None, counts=(r, r - 7)))
    return cases


# ---- softmax -------------------------------------------------------------------------------------------------------------
def _softmax_cases():
    cases = []
    lg, pr, cnt = quiet(2, 8, 2)
    rows0 = ((80, -80, -80), (80, 80, 80), (-80, 79, 80), (100, 98.5, -100), (-100, -100, -99))
    rows1 = ((-80, -80, 80), (-100, 100, 0), (80, 78, 79), (88, 89.5, 90))
    for n, rows in enumerate((rows0, rows1)):
        for r, v in enumerate(rows):
            lg[n, r, :3] = np.asarray(v, dtype=f32)
    cases.append(Case("softmax_large_logits", "logits of +-80 and +-100: exp overflows float32 (100) or its sum loses every small term unless "
                      "the row maximum is subtracted first; three equal logits of 80 give 1 / 3 twice (a tie across classes)",
                      lg, pr, np.array([8, 6], dtype=np.int32), 2))
    lg, pr, cnt = quiet(3, 8, 2)
    inf = np.inf
    rows = {0: ((-inf, 2, 0), (1, 0.5, -inf), (-inf, -inf, -inf)),
            1: ((inf, 0, 0), (3, 0, inf), (inf, inf, 0)),
            2: ((NAN, 3, 0), (3, 0, NAN), (2, NAN, 1))}
    for n, rs in rows.items():
        for r, v in enumerate(rs):
            lg[n, r, :3] = np.asarray(v, dtype=f32)
        plant(lg, pr, n, 5, 2, {0: 0.5, 1: 0.2})
        plant(lg, pr, n, 6, 2, {1: 0.4})
    cases.append(Case("softmax_nonfinite_logits", "a -inf logit in a class or in the background is a probability of 0 (row kept, its other "
                      "classes are candidates); all -inf, any +inf and any NaN logit make the row's probabilities NaN: dropped, although "
                      "the row would lead the image", lg, pr, counts(8, 7, 7), 2,
                      expect=dict(dropped=[{2: "score_not_finite"}, {0: "score_not_finite", 1: "score_not_finite", 2: "score_not_finite"},
                                           {0: "score_not_finite", 1: "score_not_finite", 2: "score_not_finite"}])))
    lg, pr, cnt = quiet(2, 16, 2)
    rng = np.random.default_rng(1100)
    lg[..., 0] = (-2.0 - rng.uniform(0, 1, (2, 16))).astype(f32)
    lg[..., 1] = (1.0 + rng.uniform(0, 1, (2, 16))).astype(f32)
    lg[..., 2] = (3.0 + rng.uniform(0, 1, (2, 16))).astype(f32)
    cases.append(Case("softmax_background_is_last", "the background (column K) is the largest logit of every row and column 0 the smallest: "
                      "read column 0 as the background and the background's 0.8 becomes a class score", lg, pr, np.array([16, 11], dtype=np.int32), 2))
    return cases


# ---- score threshold -----------------------------------------------------------------------------------------------------
def _threshold_cases():
    cases = []
    lg, pr, cnt = quiet(2, 8, 1)
    for n, (eq, near) in enumerate((((0.0, 1.5, -3.0), (1e-3, -1e-3)), ((7.0, -0.25), (2e-3, -5e-4, 1e-4)))):
        r = 0
        for a in eq:
            lg[n, r, :2] = f32(a)
            r += 1
        for e in near:
            plant(lg, pr, n, r, 1, {0: 0.5 + e})
            r += 1
        plant(lg, pr, n, r, 1, {0: 0.9})
    cases.append(Case("thresh_exact_K1", "K = 1, two equal logits: a score of exactly 1 / 2 in float32 and float64, thresh = 0.5: NOT a candidate "
                      "(score > thresh is strict); neighbours 1e-4 .. 2e-3 either side", lg, pr, counts(7, 6), 1, score_thresh=0.5, exact=True,
                      expect=dict(count=[2, 3])))
    lg, pr, cnt = quiet(2, 8, 3)
    for n, eq in enumerate(((0.0, 2.25), (-1.0, 5.0, 0.5))):
        for r, a in enumerate(eq):
            lg[n, r, :4] = f32(a)
        plant(lg, pr, n, 4, 3, {0: 0.3, 1: 0.2, 2: 0.26})
        plant(lg, pr, n, 5, 3, {1: 0.2505, 2: 0.2495})
    cases.append(Case("thresh_exact_K3", "K = 3, four equal logits: every score exactly 1 / 4, thresh = 0.25: no candidate; beside them "
                      "0.2505 (kept) and 0.2495 (not)", lg, pr, counts(8, 6), 3, score_thresh=0.25, exact=True, expect=dict(count=[3, 3])))
    lg, pr, cnt = quiet(3, 8, 2)
    t = float(f32(THRESH))
    for n in range(3):
        for r, e in enumerate((1e-4, -1e-4, 2e-5, -2e-5)):
            plant(lg, pr, n, (r + 2 * n) % 8, 2, {n % 2: t + e, 1 - n % 2: t - e * 1.5})
    cases.append(Case("thresh_neighbours", "scores 2e-5 and 1e-4 above and below thresh = 0.05 in both classes: only the ones above are candidates",
                      lg, pr, counts(4, 6, 8), 2, expect=dict(count=[4, 4, 4])))
    return cases


# ---- decode --------------------------------------------------------------------------------------------------------------
def _decode_cases():
    cases = []
    # 2 x 2 px proposals: a clamped size delta gives 125 px (62.5 x 2), inside the 300 x 420 image, so the clamp's VALUE is in
    # the output and not hidden by clipping
    lg, pr, cnt = quiet(2, 8, 2)
    values = (5 * CLAMP * (1 + 1e-3), 5 * CLAMP * (1 - 1e-3), 25.0, 1e4, np.inf, 20.0)
    for r, v in enumerate(values):
        plant(lg, pr, 0, r, 2, {0: 0.9 - 0.05 * r}, {0: (0.25, -0.5, v, 0.5)}, prop=(199, 20 + 30 * r, 201, 22 + 30 * r))
        plant(lg, pr, 1, r, 2, {1: 0.9 - 0.05 * r}, {1: (-0.5, 0.25, 0.5, v)}, prop=(20 + 40 * r, 149, 22 + 40 * r, 151))
    cases.append(Case("decode_size_clamp", "size deltas of 5 x log(1000 / 16) x (1 +- 1e-3), 25, 1e4 (unclamped, exp overflows) and +inf: d / 5 is "
                      "clamped, the box is 1000 / 16 times the proposal (125 px), finite, kept; 20 (d / 5 = 4.0, just under) is NOT clamped",
                      lg, pr, counts(6, 8), 2))
    lg, pr, cnt = quiet(2, 8, 2)
    for n in range(2):
        plant(lg, pr, n, 1 + n, 2, {n: 0.8}, {n: (0.0, 0.0, 10.0, 0.0) if n == 0 else (0.0, 0.0, 0.0, 10.0)}, prop=(200, 140, 210, 150))
        plant(lg, pr, n, 6, 2, {n: 0.6}, prop=(170, 140, 240, 150) if n == 0 else (200, 110, 210, 180))
        plant(lg, pr, n, 4, 2, {0: 0.5})
    cases.append(Case("decode_weight_then_clamp", "a size delta of 10: d / 5 = 2 lies under the clamp (e^2 = 7.4 times the size: 73.9 px, which covers "
                      "and suppresses the 70 px box of row 6); clamped BEFORE the weight it would be log(62.5) / 5 (1.2 times) and suppress nothing",
                      lg, pr, counts(8, 7), 2, expect=dict(count=[2, 2])))
    lg, pr, cnt = quiet(3, 8, 2)
    inf = np.inf
    for n, bad in enumerate(((3e38, 0, 0, 0), (0, 0, NAN, 0), (0, 0, -inf, 0))):
        plant(lg, pr, n, 0, 2, {0: 0.95}, {1: bad}, prop=(100, 100, 140, 140))
        plant(lg, pr, n, 4, 2, {0: 0.5})
        plant(lg, pr, n, 5, 2, {0: 0.4, 1: 0.3})
    plant(lg, pr, 2, 1, 2, {1: 0.9}, {0: (0, -inf, 0, 0)}, prop=(200, 100, 240, 140))
    plant(lg, pr, 0, 1, 2, {1: 0.9}, {0: (0, -3e38, 1, 1)}, prop=(200, 100, 240, 140))
    cases.append(Case("decode_nonfinite_in_subthreshold_class", "class 1 of row 0 has a score of 1e-6 and an overflowing centre delta (3e38 x 40 px: "
                      "finite in float64, not a float32), a NaN size delta or a -inf size delta, class 0 of that row is the image's best candidate: "
                      "the first two drop the WHOLE row, the third is a finite, zero-width box and drops nothing", lg, pr, counts(6, 8, 7), 2,
                      expect=dict(dropped=[{0: "box_not_finite", 1: "box_not_finite"}, {0: "box_not_finite"}, {1: "box_not_finite"}])))
    lg, pr, cnt = quiet(2, 8, 2)
    plant(lg, pr, 0, 2, 2, {0: 0.95}, {0: (3e38, 0, 0, 0)}, prop=(100, 100, 140, 140))
    plant(lg, pr, 1, 3, 2, {1: 0.95}, {1: (0, -inf, 0, 0)}, prop=(100, 100, 140, 140))
    plant(lg, pr, 1, 2, 2, {0: 0.9}, {0: (inf, 0, 0, 0)}, prop=(200, 100, 240, 140))
    for n in range(2):
        plant(lg, pr, n, 5, 2, {0: 0.5, 1: 0.3})
    cases.append(Case("decode_finite_only_after_clip", "the best candidate's own centre delta overflows (3e38), is +inf or -inf: both coordinates of "
                      "the axis are the same infinity, which clipping would turn into a finite zero-area box on the border -- the finite test "
                      "comes first and the row is dropped", lg, pr, counts(8, 6), 2, expect=dict(dropped=[{2: "box_not_finite"}, {2: "box_not_finite", 3: "box_not_finite"}])))
    return cases


# ---- clip ----------------------------------------------------------------------------------------------------------------
def _clip_cases():
    cases = []
    lg, pr, cnt = quiet(2, 13, 2)
    far = 300.0                                                   # centre delta / 10 x 20 px = 600 px
    sides = ((-far, 0), (far, 0), (0, -far), (0, far), (-far, -far))
    for n in range(2):
        for i, (dx, dy) in enumerate(sides):
            for twin in range(2):                                 # two rows with the SAME box, one class: identical zero-area boxes
                r = 2 * i + twin
                plant(lg, pr, n, r, 2, {n: 0.9 - 0.03 * r}, {n: (dx, dy, 0.0, 0.0)}, prop=(200, 140, 220, 160))
        plant(lg, pr, n, 10, 2, {n: 0.5}, prop=(200, 140, 220, 160))
        plant(lg, pr, n, 11, 2, {n: 0.45}, {n: (1.0, 0.0, 0.0, 0.0)}, prop=(200, 140, 220, 160))     # 2 px aside: suppressed by row 10
    cases.append(Case("clip_outside_zero_area", "candidates wholly left of, right of, above, below and outside a corner of the 300 x 420 image, each "
                      "twice: clipped to zero area, KEPT (no emptiness filter, unlike the RPN), and twins do not suppress each other (IoU 0 / 0)",
                      lg, pr, counts(12, 13), 2, expect=dict(count=[11, 11], zero_area=[10, 10])))
    lg, pr, cnt = quiet(2, 8, 2)
    e = 2.0 ** -6
    for n in range(2):
        plant(lg, pr, n, 0, 2, {n: 0.9}, {n: (10 * e / 20, 0, 0, 0)}, prop=(-20, 50, 0, 70))               # x2 = e
        plant(lg, pr, n, 1, 2, {n: 0.8}, {n: (0, 10 * e / 20, 0, 0)}, prop=(90, -20, 110, 0))              # y2 = e
        plant(lg, pr, n, 2, 2, {n: 0.7}, {n: (-10 * e / 20, 0, 0, 0)}, prop=(IMG_W, 120, IMG_W + 20, 140))   # x1 = img_w - e
        plant(lg, pr, n, 3, 2, {n: 0.6}, {n: (0, -10 * 3 * e / 20, 0, 0)}, prop=(150, IMG_H, 170, IMG_H + 20))   # y1 = img_h - 3 e
        plant(lg, pr, n, 4, 2, {1 - n: 0.5}, {1 - n: (0, 0, 5.0, 5.0)}, prop=(IMG_W - 30, IMG_H - 30, IMG_W - 10, IMG_H - 10))   # straddles the corner
    cases.append(Case("clip_border_slivers", "boxes that reach 2^-6 px into the image across each border (kept with that extent) and one that "
                      "straddles the bottom right corner; img_h = 300, img_w = 420: x is clipped to the width, y to the height",
                      lg, pr, counts(8, 5), 2, expect=dict(count=[5, 5])))
    return cases


# ---- order ---------------------------------------------------------------------------------------------------------------
def _order_cases():
    cases = []
    lg, pr, cnt = quiet(2, 13, 2)
    for n, rows in enumerate(((2, 5, 7, 9), (11, 0, 3, 4, 8))):
        for r in range(12):
            plant(lg, pr, n, r, 2, {0: 0.35 + 0.02 * ((r * 5) % 12), 1: 0.12 + 0.01 * ((r * 7) % 12)})
        for r in rows:
            lg[n, r] = lg[n, rows[0]]
    cases.append(Case("order_ties_across_proposals", "four (five) bit-identical logit rows among twelve: equal scores in both classes, the lower "
                      "row first", lg, pr, counts(12, 13), 2))
    lg, pr, cnt = quiet(2, 13, 3)
    for n in range(2):
        for r in range(12):
            a = 0.2 + 0.01 * ((r * 5 + n) % 12)
            plant(lg, pr, n, r, 3, {0: a, 1: 0.1 + 0.005 * r, 2: a})
            lg[n, r, 2] = lg[n, r, 0]
    cases.append(Case("order_tie_across_classes", "class 0 and class 2 of every row have the same logit: equal scores, the lower class first "
                      "(candidate id = row x K + class)", lg, pr, counts(13, 12), 3))
    k = 3
    lg, pr, cnt = quiet(2, 64, k)
    for n, (first, total) in enumerate(((62, 75), (126, 140))):
        ties = set(range(first + 1, first + 6))                   # six equal scores at ranks first .. first + 5
        scores = [0.30 - 0.0015 * min(rank, first) - 0.0015 * max(0, rank - first - 5) for rank in range(total)]
        ranked_rows(lg, n, k, scores, ties, seed=1200 + n, rows=range((40, 64)[n]))
    cases.append(Case("order_ties_straddle_chunk_edge", "six equal scores at ranks 62 .. 67 (image 0) and 126 .. 131 (image 1), every box on its "
                      "own: the tie runs across the edge of a 64-candidate chunk, lower row first on both sides of it", lg, pr, counts(40, 64), k, topk=1000,
                      expect=dict(count=[75, 140])))
    lg, pr, cnt = quiet(2, 16, 2)
    for n, first in enumerate((8, 6)):
        scores = [0.40 - 0.01 * min(rank, first) - 0.01 * max(0, rank - first - 4) for rank in range(20)]
        ranked_rows(lg, n, 2, scores, set(range(first + 1, first + 5)), seed=1210 + n, rows=range((14, 16)[n]))
    cases.append(Case("order_ties_straddle_topk", "five equal scores at ranks 8 .. 12 (6 .. 10), topk = 10: the cut falls inside the tie and "
                      "keeps its lower rows", lg, pr, counts(14, 16), 2, topk=10, expect=dict(count=[10, 10])))
    return cases


# ---- NMS -----------------------------------------------------------------------------------------------------------------
def _chain(lg, pr, n, k, rows, cls, scores, at):
    """A > B > C of 20 x 20 boxes 4 px apart: IoU(A, B) = IoU(B, C) = 16 / 24, IoU(A, C) = 12 / 28, thresh 0.5."""
    for j, (r, s) in enumerate(zip(rows, scores)):
        plant(lg, pr, n, r, k, {cls: s}, {cls: (2.0 * j, 0.0, 0.0, 0.0)}, prop=(at[0], at[1], at[0] + 20, at[1] + 20))


def _nms_cases():
    cases = []
    k = 2
    lg, pr, cnt = quiet(3, 40, k, cols=10, pitch=12)
    _chain(lg, pr, 0, k, (7, 3, 5), 0, (0.9, 0.8, 0.7), (200, 150))
    _chain(lg, pr, 0, k, (1, 2, 0), 1, (0.6, 0.5, 0.4), (300, 150))
    for n, start in ((1, 62), (2, 63)):
        # `start` singles above the chain: two to a row, then one
        scores = [0.45 - 0.003 * i for i in range(start)]
        ranked_rows(lg, n, k, scores, set(), seed=1300 + n, rows=range(0, 34))
        _chain(lg, pr, n, k, (36, 35, 38), n - 1, (0.04 * 6, 0.04 * 5, 0.04 * 4), (200, 200))
    cases.append(Case("nms_chain", "A > B > C in which A suppresses B and only B would suppress C: C survives (a suppressed box suppresses "
                      "nothing); at the top of the list, and at ranks 62-63-64 and 63-64-65 across the first chunk edge", lg, pr, counts(9, 40, 39), k, topk=1000))
    lg, pr, cnt = quiet(2, 8, 2)
    for n in range(2):
        d = (0.5, -0.5, 0.3, 0.2)
        plant(lg, pr, n, 2 + n, 2, {0: 0.5, 1: 0.4}, {0: d, 1: d}, prop=(100, 100, 140, 130))
        plant(lg, pr, n, 5, 2, {0: 0.3, 1: 0.35}, {0: d, 1: d}, prop=(102, 101, 142, 131))
    cases.append(Case("nms_same_box_two_classes", "the same box in class 0 and class 1 (both kept: classes never meet), and a second row on top "
                      "of it that is suppressed once in each class", lg, pr, counts(8, 6), 2, expect=dict(count=[2, 2])))
    c60 = np.zeros((2, 32, 2), dtype=bool)
    c60[:, :30] = True
    cases.append(dense_case("nms_clusters_in_one_chunk", "60 candidates in 5 (7) clusters, two classes: everything is resolved inside the first "
                            "64-candidate chunk", 1310, 32, 2, c60, 0.1, 0.45, (5, 7), counts=(32, 30), expect=dict(count=[10, 14])))
    c = dense_case("nms_clusters_from_earlier_chunk", "192 candidates in 6 clusters, three classes; the 18 leaders hold the 18 best scores: "
                   "chunks 1 and 2 are suppressed from the kept list alone", 1311, 64, 3, np.ones((2, 64, 3), dtype=bool), 0.06, 0.3, 6,
                   counts=(64, 50), expect=dict(count=[18, 18]))
    for n in range(2):
        for cl in range(6):
            x, y = 8.0 + 24 * cl, 8.0                               # cluster cl's own place
            plant(c.logits, c.props, n, cl, 3, {0: 0.32 - 0.001 * cl, 1: 0.3145 - 0.001 * cl, 2: 0.3085 - 0.001 * cl}, prop=(x, y, x + 16, y + 16))
    cases.append(c)
    for m, seed in ((63, 1320), (64, 1321), (65, 1322), (128, 1323), (129, 1324)):
        rng = np.random.default_rng(seed)
        cand = np.zeros((2, 64 * 3), dtype=bool)
        cand[0, rng.permutation(192)[:m]] = True
        cand[1, rng.permutation(150)[:m]] = True
        cases.append(dense_case(f"ncand_{m}", f"exactly {m} candidates in 12 clusters: "
                                + {63: "one short of a chunk", 64: "one full chunk", 65: "one candidate in the second chunk", 128: "two full chunks",
                                   129: "one candidate in the third chunk"}[m], seed, 64, 3, cand.reshape(2, 64, 3), 0.06, 0.3, 12, counts=(64, 50),
                                topk=1000, expect=dict(ncand=[m, m])))
    for which in ("at", "below"):
        lg, pr, cnt = quiet(2, 8, 2)
        # image 0: 48 x 48 squares 16 px apart: 32 x 48 / (2 x 2304 - 1536) = 1 / 2; image 1: 24 x 24, 8 px: 16 x 24 / (1152 - 384)
        for n, (size, step) in enumerate(((48, 16), (24, 8))):
            for cl in range(2):
                x, y = 40 + 150 * cl, 60 + 100 * n
                plant(lg, pr, n, 1 + 3 * cl, 2, {cl: 0.6 - 0.1 * cl}, prop=(x, y, x + size, y + size))
                plant(lg, pr, n, 2 + 3 * cl, 2, {cl: 0.3 + 0.1 * cl}, prop=(x + step, y, x + step + size, y + size))
        thr = f32(0.5) if which == "at" else np.nextafter(f32(0.5), f32(0))
        cases.append(Case(f"nms_iou_exactly_half_{which}", "pairs of integer boxes with IoU exactly 1 / 2 (also after the integer shift by class x "
                          "(max + 1)), nms_thresh " + ("equal to it: kept (strict >)" if which == "at" else "one float below it: suppressed"),
                          lg, pr, counts(8, 6), 2, nms_thresh=float(thr), exact=True, expect=dict(count=[4, 4] if which == "at" else [2, 2])))
    return cases


# ---- regimes and capacity ------------------------------------------------------------------------------------------------
def _regime_cases():
    cases = []
    cases.append(dense_case("regime_1000_candidates", "K = 1, exactly 1000 candidates (4 x 1000 coordinates <= 4000: the shifted-coordinate NMS) "
                            "beside an image of 700", 1400, 1000, 1, np.ones((2, 1000, 1), dtype=bool), 0.1, 0.9, (50, 37), counts=(1000, 700),
                            expect=dict(ncand=[1000, 700])))
    cases.append(dense_case("regime_1001_candidates", "K = 1, exactly 1001 candidates (one NMS per class on the plain boxes) beside an image of "
                            "exactly 1000", 1401, 1001, 1, np.ones((2, 1001, 1), dtype=bool), 0.1, 0.9, (50, 37), counts=(1001, 1000),
                            expect=dict(ncand=[1001, 1000])))
    cand = np.ones((2, 501, 2), dtype=bool)
    cand[0, 500, 1] = False                                       # 1001
    cand[1, 500] = False                                          # 1000
    cases.append(dense_case("regime_1001_candidates_K2", "two classes, 1001 candidates beside 1000: on the left of the switch class 1 is shifted "
                            "by max + 1, on the right it is not", 1402, 501, 2, cand, 0.1, 0.45, (40, 33), counts=(501, 500), expect=dict(ncand=[1001, 1000])))
    # one low candidate alone holds the maximum coordinate
    c = dense_case("regime_max_coordinate_from_low_candidate", "three classes, 182 candidates inside 0 .. 200 px whose boxes coincide across the "
                   "classes, a class-1 box at 649 .. 699 and the LOWEST score of the image, class 0, alone at 850 .. 900: boxes.max() is taken over "
                   "all candidates (901 per class); taken short of the last one (max = 699) the class-1 box would be shifted onto it",
                   1403, 62, 3, np.ones((2, 62, 3), dtype=bool), 0.08, 0.3, (20, 14), counts=(62, 47), same_deltas=True, img=(950, 1000),
                   expect=dict(ncand=[182, 137]))
    for n, last in enumerate((61, 46)):
        c.logits[n, last, 4:] = 0
        c.logits[n, last - 1, 4:] = 0
        plant(c.logits, c.props, n, last, 3, {0: 0.06}, prop=(850, 850, 900, 900))
        plant(c.logits, c.props, n, last - 1, 3, {1: 0.5}, prop=(649, 649, 699, 699))
    cases.append(c)
    cases.append(dense_case("capacity_4096", "R = 1024, K = 4, thresh = 0.2 and four scores above 0.2 in every row: 4096 candidates, every slot of "
                            "the sort is taken and all 64 chunks are walked (160 kept < topk); beside it an image of 1000 rows (4000 candidates)",
                            1410, 1024, 4, np.ones((2, 1024, 4), dtype=bool), 0.2005, 0.2455, (40, 31), counts=(1024, 1000), score_thresh=0.2, topk=1000,
                            expect=dict(ncand=[4096, 4000], count=[160, 124])))
    return cases


# ---- top-k ---------------------------------------------------------------------------------------------------------------
def _topk_cases():
    cases = []
    full = np.ones((2, 64, 3), dtype=bool)

    def lone(name, why, topk, seed=1500, **kw):                   # every row a cluster of its own: 192 (150) candidates, all kept
        return dense_case(name, why, seed, 64, 3, full, 0.06, 0.3, 64, counts=(64, 50), topk=topk, **kw)

    def clustered(name, why, topk, seed=1501, **kw):
        return dense_case(name, why, seed, 64, 3, full, 0.06, 0.3, (9, 5), counts=(64, 50), topk=topk, **kw)

    cases.append(lone("topk_1", "topk = 1: the best candidate of each image only", 1, expect=dict(count=[1, 1])))
    least = min(r["survivors"] for r in _ref(clustered("", "", 1000)))
    assert least == 15
    cases.append(clustered("topk_equal_kept", "topk = 15, the survivor count of image 1 (image 0 has 27): the list is exactly full", least, expect=dict(count=[15, 15])))
    cases.append(clustered("topk_kept_minus_one", "topk = 14: one below image 1's survivor count, its last survivor is cut", least - 1, expect=dict(count=[14, 14])))
    cases.append(lone("topk_128", "topk = 128 = DET_WAVE0K with 192 / 150 survivors: the longest list of the one-wave path, full", 128, expect=dict(count=[128, 128])))
    cases.append(lone("topk_129", "topk = 129: the shortest list of the sixteen-wave path, full", 129, expect=dict(count=[129, 129])))
    cases.append(lone("topk_1000_many_kept", "topk = 1000 with 192 / 150 survivors: more than 128 kept boxes are scanned by waves 1 .. 15", 1000,
                      expect=dict(count=[192, 150])))
    cases.append(clustered("topk_1000_few_kept", "topk = 1000 with 27 / 15 survivors: most waves of the sixteen have no kept box to scan", 1000,
                           expect=dict(count=[27, 15])))
    cases.append(lone("topk_cut_mid_chunk", "topk = 100 with every candidate kept: chunk 0 gives 64 rows, the cut falls at lane 36 of chunk 1", 100,
                      seed=1502, expect=dict(count=[100, 100])))
    cases.append(dense_case("topk_cut_mid_chunk_after_suppression", "topk = 40 over 16 / 14 clusters in three classes: chunk 0 keeps fewer than 40, the "
                            "cut falls among the survivors of chunk 1", 1503, 64, 3, full, 0.06, 0.3, (16, 14), counts=(64, 50), topk=40,
                            expect=dict(count=[40, 40])))
    return cases


def _random_cases():
    return [random_case(f"random_{i}", "seeded random logits, deltas and clustered proposals, K = 3, production thresholds", seed, 3, 48, 3,
                        counts=(48, 31, 40), ld=16 + 4 * i) for i, seed in enumerate((1600, 1604, 1606))]


CASES = (_row_cases() + _softmax_cases() + _threshold_cases() + _decode_cases() + _clip_cases() + _order_cases() + _nms_cases()
         + _regime_cases() + _topk_cases() + _random_cases())
NAMES = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
for _c in CASES:
    for _a in (_c.logits, _c.props, _c.prop_count):
        _a.setflags(write=False)

_REFS = {}


def reference(case: Case) -> list:
    """The reference's result for every image of ``case``: computed once, shared, read only."""
    if case.name not in _REFS:
        res = _ref(case)
        for r in res:
            for k in ("boxes", "scores", "classes", "src", "S"):
                r[k].setflags(write=False)
        _REFS[case.name] = res
    return _REFS[case.name]
