"""The box-detection reference and its case table, checked without a GPU.

  * every case of ``box_dets_cases.py`` keeps the reference's decisions away from their thresholds (the condition the GPU
    test rests on: no kept set or order of the table can depend on float32 against float64 rounding), except the cases
    marked ``exact``, which sit ON a threshold with values exact in both precisions;
  * every case does what it is named for, by the reference's own record, and the hand-computed anchors hold: a score of
    exactly 1 / 2 or 1 / 4 is no candidate, the clamp gives 1000 / 16 times the size, boxes clipped to zero area survive;
  * what float32 costs: ``dets_f32`` (float32 throughout, one rounding per operation) keeps the reference's rows in the
    reference's order on every case, and its distance from the float64 scores and boxes is the MEASUREMENT the GPU bars
    are derived from -- printed, and held to its records ``F32_VS_REF_SCORE`` and ``F32_VS_REF_BOX``;
  * the reference can see mistakes: fourteen mutants of it each change the kept set, order or count of a named case.
"""
import numpy as np

import box_dets_cases as T
import box_dets_ref as REF

ULP = 2.0 ** -24
MIN_SCORE_MARGIN = 16 * T.F32_VS_REF_SCORE * ULP


def _worst(c, key):
    return min(r["margins"][key] for r in T.reference(c))


def test_every_case_keeps_its_decisions_away_from_the_thresholds():
    bad = []
    for c in T.CASES:
        res = T.reference(c)
        m = {k: _worst(c, k) for k in ("score", "gap", "iou", "iou_rel", "finite")}
        flips = sum(r["margins"]["iou_flips"] for r in res)
        ties = sum(r["margins"]["tie_mismatch"] for r in res)
        print(f"{c.name:42s} N {c.n_images} R {c.R:4d} K {c.K} ld {c.ld:2d}  candidates {[r['ncand'] for r in res]}  kept {[r['count'] for r in res]}  "
              f"min |score - thr| {m['score']:.1e}  score gap {m['gap']:.1e}  |IoU - thr| {m['iou']:.1e} = {m['iou_rel']:.1e} x its f32 error  "
              f"finite test {m['finite']:.1f} binades")
        if c.exact:
            if not (m["score"] == 0.0 or m["iou"] <= 6e-8):
                bad.append((c.name, "marked exact but nothing sits on a threshold", m["score"], m["iou"]))
        else:
            if m["score"] < MIN_SCORE_MARGIN:
                bad.append((c.name, "score margin", m["score"]))
            if m["iou"] < T.MIN_IOU_MARGIN:
                bad.append((c.name, "IoU margin", m["iou"]))
        if m["gap"] < MIN_SCORE_MARGIN:
            bad.append((c.name, "score gap", m["gap"]))
        if m["iou_rel"] < 16:
            bad.append((c.name, "IoU margin against that pair's float32 error", m["iou_rel"]))
        if flips:
            bad.append((c.name, "pairs that float64, float32 and shifted float32 decide differently", flips))
        if ties:
            bad.append((c.name, "score ties that are not bit-equal in both precisions", ties))
        if m["finite"] < T.MIN_FINITE_MARGIN:
            bad.append((c.name, "finite-test margin", m["finite"]))
    assert not bad, bad
    assert sorted(c.name for c in T.CASES if c.exact) == ["nms_iou_exactly_half_at", "nms_iou_exactly_half_below", "thresh_exact_K1", "thresh_exact_K3"]


def _has(r, row, cls):
    return bool((r["src"] == np.array([row, cls])).all(axis=1).any())


def _area(r):
    b = r["boxes"][:r["count"]]
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def test_every_named_case_does_what_it_is_named_for():
    ref = {c.name: T.reference(c) for c in T.CASES}
    for c in T.CASES:
        assert 2 <= c.n_images <= 5 and (c.R <= 64 or c.name.startswith(("regime_100", "capacity_"))), c.name
        assert len(set(c.prop_count.tolist())) > 1, (c.name, "every image has the same prop_count")
        assert c.logits.dtype == np.float32 and c.props.dtype == np.float32 and c.prop_count.dtype == np.int32, c.name
        for key in ("count", "ncand", "dropped"):
            if key in c.expect:
                assert [r[key] for r in ref[c.name]] == c.expect[key], (c.name, key, [r[key] for r in ref[c.name]])
        for n, r in enumerate(ref[c.name]):
            assert r["count"] == min(c.topk, r["survivors"]) and not r["boxes"][r["count"]:].any() and not r["scores"][r["count"]:].any(), (c.name, n)
            assert (r["src"][:, 0] < min(int(c.prop_count[n]), c.R)).all(), (c.name, n, "a row past prop_count was used")
    # rows and strides
    assert T.BY_NAME["rows_prop_count_edges"].prop_count.tolist() == [0, 1, 15, 16, 21] and T.BY_NAME["rows_prop_count_edges"].R == 16
    assert ref["rows_prop_count_edges"][0]["count"] == 0 and all(r["count"] > 0 for r in ref["rows_prop_count_edges"][1:])
    c = T.BY_NAME["rows_past_count_hold_nan_and_best_scores"]
    for n, cnt in enumerate(c.prop_count):
        tail = c.logits[n, cnt:, :3]
        best = np.nanmax(REF.softmax(tail, np.float64)[:, :2])
        assert np.isnan(tail).any() and best > REF.softmax(c.logits[n, :cnt, :3], np.float64)[:, :2].max(), (n, "the rows past the count must hold NaN and the best score")
    assert [(T.BY_NAME[n].K, T.BY_NAME[n].ld) for n in ("ld_exact_odd_K", "ld_exact_even_K", "ld_padded_garbage", "classes_K8")] == [(3, 16), (2, 11), (2, 16), (8, 44)]
    for n in ("ld_padded_garbage", "classes_K8", "random_1", "random_2"):
        c = T.BY_NAME[n]
        assert np.abs(c.logits[..., 5 * c.K + 1:]).min() > 1e37, (n, "the pad columns must hold junk")
    assert [T.BY_NAME[f"classes_K{k}"].K for k in (1, 2, 3, 5, 8)] == [1, 2, 3, 5, 8]
    for k in (2, 3, 5, 8):
        assert all(len(set(r["classes"][:r["count"]].tolist())) == k for r in ref[f"classes_K{k}"]), (k, "not every class is detected")
    # softmax
    big = T.BY_NAME["softmax_large_logits"].logits[..., :3]
    assert np.abs(big).max() == 100 and (np.abs(big) == 80).any()
    r = ref["softmax_large_logits"][0]
    assert r["scores"][0] == 1.0 and _has(r, 1, 0) and _has(r, 1, 1)
    i = [int(j) for j in np.nonzero(r["src"][:, 0] == 1)[0]]
    assert r["scores"][i[0]] == r["scores"][i[1]] == 1.0 / 3.0 and r["classes"][i[0]] == 0 and i[1] == i[0] + 1
    r = ref["softmax_nonfinite_logits"]
    assert _has(r[0], 0, 1) and _has(r[0], 1, 0) and _has(r[0], 1, 1) and not _has(r[0], 0, 0)
    assert all(x["count"] == 3 for x in r[1:]), "only the ordinary rows of the +inf and the NaN image survive"
    c = T.BY_NAME["softmax_background_is_last"]
    assert (c.logits[..., :3].argmax(axis=2) == 2).all() and (c.logits[..., :3].argmin(axis=2) == 0).all()
    # threshold: hand-computed anchors
    for name, k, rows in (("thresh_exact_K1", 1, ((0, 1, 2), (0, 1))), ("thresh_exact_K3", 3, ((0, 1), (0, 1, 2)))):
        c = T.BY_NAME[name]
        assert c.score_thresh == 1.0 / (k + 1)
        for n, rs in enumerate(rows):
            for row in rs:
                assert len(set(c.logits[n, row, :k + 1].tolist())) == 1, (name, n, row, "the logits of the row must be equal")
                for dt in (np.float32, np.float64):
                    p = REF.softmax(c.logits[n, row:row + 1, :k + 1], dt)
                    assert (p == dt(c.score_thresh)).all(), (name, n, row, dt)
                assert not any(_has(ref[name][n], row, cl) for cl in range(k)), (name, n, row, "a score ON the threshold became a candidate")
    assert all(r["ncand"] == 4 for r in ref["thresh_neighbours"])
    # decode: the clamp gives 1000 / 16 times the 2 px proposal
    r = ref["decode_size_clamp"]
    w0 = r[0]["boxes"][:6, 2] - r[0]["boxes"][:6, 0]
    h1 = r[1]["boxes"][:6, 3] - r[1]["boxes"][:6, 1]
    for ext in (w0, h1):
        assert ext[0] == ext[2] == ext[3] == ext[4] and abs(ext[0] - 125.0) < 1e-9, ext           # above the clamp, 25, 1e4, +inf: 2 px x 62.5
        assert ext[0] * np.exp(-1.001e-3 * REF.SCALE_CLAMP) < ext[1] < ext[0] * np.exp(-0.999e-3 * REF.SCALE_CLAMP), ext
        assert abs(ext[5] - 2.0 * np.exp(4.0)) < 1e-9, ext                                        # 20 / 5 = 4.0: under the clamp
    r = ref["decode_weight_then_clamp"]
    assert abs((r[0]["boxes"][0, 2] - r[0]["boxes"][0, 0]) - 10.0 * np.exp(2.0)) < 1e-9 and abs((r[1]["boxes"][0, 3] - r[1]["boxes"][0, 1]) - 10.0 * np.exp(2.0)) < 1e-9
    r = ref["decode_nonfinite_in_subthreshold_class"]
    assert not _has(r[0], 0, 0) and not _has(r[1], 0, 0) and r[2]["src"][0].tolist() == [0, 0] and r[2]["scores"][0] > 0.94
    r = ref["decode_finite_only_after_clip"]
    assert all(x["count"] == 2 and (_area(x) > 0).all() for x in r)
    # clip: zero-area survivors
    for n, x in enumerate(ref["clip_outside_zero_area"]):
        a = _area(x)
        assert int((a == 0).sum()) == 10 and x["count"] == 11, (n, a)
        b = x["boxes"][:10]
        assert sorted(map(tuple, b.tolist())) == sorted([(0, 140, 0, 160)] * 2 + [(420, 140, 420, 160)] * 2 + [(200, 0, 220, 0)] * 2
                                                        + [(200, 300, 220, 300)] * 2 + [(0, 0, 0, 0)] * 2), b
        assert not _has(x, 11, n)
    for x in ref["clip_border_slivers"]:
        b = x["boxes"]
        assert abs(b[0, 2] - 2.0 ** -6) < 1e-9 and abs(b[1, 3] - 2.0 ** -6) < 1e-9 and abs(420 - b[2, 0] - 2.0 ** -6) < 1e-7 and abs(300 - b[3, 1] - 3 * 2.0 ** -6) < 1e-7
        assert b[4, 2] == 420 and b[4, 3] == 300 and 0 < b[4, 0] < 390 and 0 < b[4, 1] < 270
    c = T.BY_NAME["clip_border_slivers"]
    assert c.img_h != c.img_w
    # order
    for n, rows in enumerate(((2, 5, 7, 9), (11, 0, 3, 4, 8))):
        x = ref["order_ties_across_proposals"][n]
        for cl in range(2):
            got = [int(s[0]) for s in x["src"] if s[1] == cl and s[0] in rows]
            at = [i for i, s in enumerate(x["src"]) if s[1] == cl and s[0] in rows]
            assert got == sorted(rows) and at == list(range(at[0], at[0] + len(rows))), (n, cl, got, at)
    for x in ref["order_tie_across_classes"]:
        for row in range(12):
            i = [int(j) for j in np.nonzero((x["src"][:, 0] == row) & (x["src"][:, 1] != 1))[0]]
            assert x["src"][i[0], 1] == 0 and x["src"][i[1], 1] == 2 and x["scores"][i[0]] == x["scores"][i[1]], row
    for name, firsts, length in (("order_ties_straddle_chunk_edge", (62, 126), 6), ("order_ties_straddle_topk", (8, 6), 5)):
        for n, first in enumerate(firsts):
            x = REF.detections_one_image(T.BY_NAME[name].logits[n], T.BY_NAME[name].props[n], int(T.BY_NAME[name].prop_count[n]), T.BY_NAME[name].K, T.IMG_H, T.IMG_W,
                                         T.THRESH, 0.5, 1000)
            s = x["scores"][:x["count"]]
            assert (s[first:first + length] == s[first]).all() and s[first - 1] > s[first] > s[first + length], (name, n)
            assert (np.diff(x["src"][first:first + length, 0]) > 0).all(), (name, n, "equal scores: lower row first")
            assert (np.diff(x["src"][:first, 0]) < 0).any(), (name, n, "rank and row number must be unrelated")
    # NMS
    x = ref["nms_chain"]
    assert _has(x[0], 7, 0) and not _has(x[0], 3, 0) and _has(x[0], 5, 0) and _has(x[0], 1, 1) and not _has(x[0], 2, 1) and _has(x[0], 0, 1)
    for n, start in ((1, 62), (2, 63)):
        assert _has(x[n], 36, n - 1) and not _has(x[n], 35, n - 1) and _has(x[n], 38, n - 1)
        assert x[n]["rank"][-2:].tolist() == [start, start + 2], (n, x[n]["rank"][-3:])
    for x in ref["nms_same_box_two_classes"]:
        assert x["count"] == 2 and (x["boxes"][0] == x["boxes"][1]).all() and x["classes"][:2].tolist() == [0, 1] and x["src"][0, 0] == x["src"][1, 0]
    for x in ref["nms_clusters_in_one_chunk"]:
        assert x["ncand"] == 60
    for x in ref["nms_clusters_from_earlier_chunk"]:
        assert sorted(x["rank"].tolist()) == list(range(18)) and x["ncand"] > 128
    for m in (63, 64, 65, 128, 129):
        assert all(r["ncand"] == m and r["count"] < r["ncand"] for r in ref[f"ncand_{m}"])
    at, below = T.BY_NAME["nms_iou_exactly_half_at"], T.BY_NAME["nms_iou_exactly_half_below"]
    assert at.nms_thresh == 0.5 and below.nms_thresh == float(np.nextafter(np.float32(0.5), np.float32(0)))
    assert all((c.props == np.round(c.props)).all() and not c.logits[..., 3:].any() for c in (at, below)), "integer boxes, zero deltas"
    # regimes and capacity
    assert [r["ncand"] for r in ref["regime_1000_candidates"] + ref["regime_1001_candidates"]] == [1000, 700, 1001, 1000]
    assert T.BY_NAME["regime_1000_candidates"].K == T.BY_NAME["regime_1001_candidates"].K == 1
    c = T.BY_NAME["regime_max_coordinate_from_low_candidate"]
    for n, x in enumerate(ref[c.name]):
        last = int(c.prop_count[n]) - 1
        assert x["ncand"] <= 1000 and x["max_coord_holders"] == 1 and x["max_coord_src"] == (last, 0)
        assert x["src"][-1].tolist() == [last, 0] and x["boxes"][x["count"] - 1].tolist() == [850, 850, 900, 900], "the lowest score holds the maximum coordinate"
        assert _has(x, last - 1, 1)
        b = x["boxes"][:x["count"]]
        twins = sum(1 for i in range(x["count"]) for j in range(i) if (b[i] == b[j]).all() and x["classes"][i] != x["classes"][j])
        assert twins >= 10, (n, twins, "boxes of different classes must coincide")
    c = T.BY_NAME["capacity_4096"]
    assert (c.R, c.K, c.score_thresh) == (1024, 4, 0.2) and c.R * min(c.K, int(np.float32(1) / np.float32(c.score_thresh))) == 4096
    assert ref[c.name][0]["ncand"] == 4096 and ref[c.name][0]["count"] < c.topk
    # top-k
    assert [T.BY_NAME[n].topk for n in ("topk_1", "topk_128", "topk_129", "topk_1000_many_kept", "topk_1000_few_kept")] == [1, 128, 129, 1000, 1000]
    assert min(r["survivors"] for r in ref["topk_equal_kept"]) == T.BY_NAME["topk_equal_kept"].topk == T.BY_NAME["topk_kept_minus_one"].topk + 1
    assert all(r["survivors"] > 129 for r in ref["topk_129"]) and all(r["survivors"] < 128 for r in ref["topk_1000_few_kept"])
    for x in ref["topk_cut_mid_chunk"]:
        assert x["rank"].tolist() == list(range(100))
    for x in ref["topk_cut_mid_chunk_after_suppression"]:
        assert int((x["rank"] < 64).sum()) < 40 and 64 < x["rank"][-1] < 128 and x["survivors"] > 40, (x["rank"], "the cut must fall among the survivors of chunk 1")
    assert sum(n.startswith("random_") for n in T.NAMES) == 3


def test_float32_restatement_against_the_reference_is_the_recorded_figures():
    worst_s, worst_b = (0.0, None), (0.0, None)
    bad = []
    for c in T.CASES:
        for n, r in enumerate(T.reference(c)):
            g = REF.dets_f32(c.logits[n], c.props[n], int(c.prop_count[n]), c.K, c.img_h, c.img_w, c.score_thresh, c.nms_thresh, c.topk)
            k = r["count"]
            if g["count"] != k or not np.array_equal(g["src"], r["src"]):
                bad.append((c.name, n, "float32 keeps other rows or another order", g["count"], k))
                continue
            if k == 0:
                continue
            es = np.abs(g["scores"].astype(np.float64) - r["scores"][:k]) / ULP
            S = np.stack([r["S"][:, 0], r["S"][:, 1]] * 2, axis=1)
            eb = np.abs(g["boxes"].astype(np.float64) - r["boxes"][:k]) / (ULP * S)
            if es.max() > worst_s[0]:
                worst_s = (float(es.max()), (c.name, n, int(es.argmax())))
            i = np.unravel_index(int(eb.argmax()), eb.shape)
            if eb[i] > worst_b[0]:
                worst_b = (float(eb[i]), (c.name, n, int(i[0]), int(i[1])))
    print(f"largest |float32 score - reference| = {worst_s[0]:.3f} x 2^-24 at {worst_s[1]}; record {T.F32_VS_REF_SCORE} at {T.F32_VS_REF_SCORE_AT}, "
          f"GPU bar {4 * T.F32_VS_REF_SCORE} x 2^-24")
    print(f"largest |float32 box - reference| = {worst_b[0]:.3f} x 2^-24 S at {worst_b[1]}; record {T.F32_VS_REF_BOX} at {T.F32_VS_REF_BOX_AT}, "
          f"GPU bar {4 * T.F32_VS_REF_BOX} x 2^-24 S")
    assert not bad, bad
    # (numpy's float32 exp may differ by an ulp from one CPU to the next: a quarter more)
    for worst, record in ((worst_s, T.F32_VS_REF_SCORE), (worst_b, T.F32_VS_REF_BOX)):
        assert worst[0] <= 1.25 * record, worst
        assert worst[0] >= record / 2, ("the record is stale: measure again", worst)


# the cases each mutant is tried on: the small ones built for the rule it breaks (all fourteen mutants run on all of them)
MUTANT_CASES = ("softmax_background_is_last", "thresh_exact_K1", "thresh_exact_K3", "nms_iou_exactly_half_at", "nms_same_box_two_classes", "nms_chain",
                "decode_nonfinite_in_subthreshold_class", "decode_finite_only_after_clip", "decode_size_clamp", "decode_weight_then_clamp",
                "clip_outside_zero_area", "order_ties_across_proposals", "order_tie_across_classes", "order_ties_straddle_topk",
                "topk_kept_minus_one", "rows_past_count_hold_nan_and_best_scores", "rows_prop_count_edges")
BUILT_FOR = {"background_first": "softmax_background_is_last", "threshold_greater_equal": "thresh_exact_K1", "nms_greater_equal": "nms_iou_exactly_half_at",
             "nms_across_classes": "nms_same_box_two_classes", "suppressed_still_suppress": "nms_chain", "drop_class_not_row": "decode_nonfinite_in_subthreshold_class",
             "clip_before_finite_test": "decode_finite_only_after_clip", "no_clamp": "decode_size_clamp", "clamp_before_weight": "decode_weight_then_clamp",
             "weights_swapped": "decode_weight_then_clamp", "drop_empty_boxes": "clip_outside_zero_area", "tie_order_reversed": "order_ties_across_proposals",
             "topk_before_nms": "topk_kept_minus_one", "rows_past_count_used": "rows_past_count_hold_nan_and_best_scores"}


def _differs(got, ref):
    """Kept set, order or count: nothing that only a tolerance could tell."""
    return any(g["count"] != r["count"] or not np.array_equal(g["src"], r["src"]) for g, r in zip(got, ref))


def test_the_reference_notices_each_of_fourteen_mistakes():
    assert set(BUILT_FOR) == set(REF.MUTANTS) and len(REF.MUTANTS) == 14
    caught = {m: [] for m in REF.MUTANTS}
    for name in MUTANT_CASES:
        c = T.BY_NAME[name]
        ref = T.reference(c)
        for m in REF.MUTANTS:
            got = REF.detections(c.logits, c.props, c.prop_count, c.K, c.img_h, c.img_w, c.score_thresh, c.nms_thresh, c.topk, mutant=m)
            if _differs(got, ref):
                caught[m].append(name)
    for m in REF.MUTANTS:
        print(f"mutant {m:26s} caught by: {', '.join(caught[m]) or 'NOTHING'}")
    for m in REF.MUTANTS:
        assert BUILT_FOR[m] in caught[m], f"mutant {m} does not change the kept set, order or count of {BUILT_FOR[m]}, the case built for it (it changes: {caught[m]})"
