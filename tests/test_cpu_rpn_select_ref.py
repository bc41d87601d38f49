"""The RPN proposal-selection reference and its case table, checked without a GPU.

  * every case of ``rpn_select_cases.py`` keeps the reference's decisions away from their thresholds (the condition the
    GPU test rests on: no kept set of the table can depend on float32 against float64 rounding), except the cases marked
    ``exact``, which sit ON the NMS threshold with integer geometry;
  * every case does what it is named for, by the reference's own record;
  * the reference (``rpn_select_ref.py``: numpy, float64 boxes) agrees with the oracle's float32 building blocks
    (``oracle.maskrcnn_ref``: ``grid_anchors``, ``apply_deltas``, ``nms``, ``batched_nms``, assembled as ``rpn_forward``
    assembles them) on kept rows, order and count of every case and image, NaN size deltas included (``torch.clamp``
    propagates NaN, as the reference does), and on the boxes within the GPU test's bar;
  * what float32 costs: the decode restated in float32, one rounding per operation, against the float64 decode -- the
    MEASUREMENT the GPU bar is derived from, printed, and held to its record ``rpn_select_cases.F32_VS_REF``;
  * the reference can see mistakes: seven mutants of it each change the result of a named case.
"""
import numpy as np
import pytest
import torch

import rpn_select_cases as T
import rpn_select_ref as REF

ULP = 2.0 ** -24


def test_every_case_keeps_its_decisions_away_from_the_thresholds():
    bad = []
    for c in T.CASES:
        res = T.reference(c)
        m = {k: min(r["margins"][k] for r in res) for k in ("iou", "extent", "empty")}
        print(f"{c.name:36s} images {c.n_images}  rows {[r['count'] for r in res]}  survivors {[r['survivors'] for r in res]}  "
              f"min |IoU - thr| {m['iou']:.2e}  min extent {m['extent']:.2e} px  min emptying distance {m['empty']:.2e} px")
        if c.exact:
            if not m["iou"] <= 6e-8:
                bad.append((c.name, "marked exact but no pair sits on the threshold", m["iou"]))
        elif m["iou"] < T.MIN_IOU_MARGIN:
            bad.append((c.name, "IoU margin", m["iou"]))
        if m["extent"] < T.MIN_PX_MARGIN or m["empty"] < T.MIN_PX_MARGIN:
            bad.append((c.name, "pixel margin", m["extent"], m["empty"]))
    assert not bad, bad
    assert sorted(c.name for c in T.CASES if c.exact) == sorted(n for n in T.NAMES if n.startswith("nms_thresh_exactly_"))


def _rows(r):
    """(level, score) of the output rows, in order."""
    return [(int(s[0]), float(v)) for s, v in zip(r["src"], r["scores"][:r["count"]])]


def _has(r, lv, h, w, a):
    return bool((r["src"] == np.array([lv, h, w, a])).all(axis=1).any())


def test_every_named_case_does_what_it_is_named_for():
    ref = {c.name: T.reference(c) for c in T.CASES}
    # selection: a level above pre_topk and levels below it; ties at the cut; both sides of the candidate list's capacity
    sm = T.BY_NAME["select_smooth"]
    assert [h.shape[1] * h.shape[2] * 3 for h in sm.heads] == [1440, 450, 90, 27, 3] and sm.pre_topk == 1000
    q = T.BY_NAME["select_quantised"].heads[0][0, :, :, :3].reshape(-1)
    cut = np.sort(q)[::-1][999]
    assert (q == cut).sum() >= 100 and (q > cut).sum() < 1000 < (q >= cut).sum(), "no tie group straddles the cut"
    for name, lo, hi in (("select_overflow", 8193, 9408), ("select_one_bin_fits", 8000, 8192)):
        lg = T.BY_NAME[name].heads[0][..., :3]
        assert lo <= lg[0].size <= hi and lg.min() >= 1.0 and lg.max() < 1.125, name       # one bin of (sign, exponent, 3 mantissa bits)
    two = T.BY_NAME["select_two_bins"].heads[0][0, :, :, :3]
    assert 1000 < (two >= 1.0).sum() <= 8192 and (two < 1.0).sum() > 1000
    sg = T.BY_NAME["select_signs_and_extremes"]
    for n in range(2):
        lg = sg.heads[0][n, :, :, :3].reshape(-1)
        pz, nz = np.nonzero((lg == 0) & ~np.signbit(lg))[0], np.nonzero((lg == 0) & np.signbit(lg))[0]
        assert pz.size == 50 and nz.size == 50 and pz.max() < nz.min(), "+0.0 must lie at lower indices than -0.0"
        assert (lg > 0).sum() + np.isnan(lg).sum() < 900 and (lg >= 0).sum() + np.isnan(lg).sum() < 900, "zeros must stay off the cut"
        assert np.isnan(lg).sum() == 3 and not np.signbit(lg[np.isnan(lg)]).any() and np.isposinf(lg).sum() == 4 and np.isneginf(lg).sum() == 20
        s = ref[sg.name][n]["scores"][:ref[sg.name][n]["count"]]
        assert (s == 0).sum() > 10 and np.signbit(s[s == 0]).any() and not np.signbit(s[s == 0]).all(), "both zeros must reach the output"
        assert ref[sg.name][n]["dropped"]["not_finite"] == 3 + 4 + 2 + 2 + 5
    for c in T.CASES:                                                            # -0.0 logits nowhere else (its order against +0.0 is not specified)
        if c.name != sg.name:
            assert not any(((h[..., :3] == 0) & np.signbit(h[..., :3])).any() for h in c.heads), c.name
    # top-k parameters
    for k in (1, 63, 64, 65, 1000):
        assert T.BY_NAME[f"pre_topk_{k}"].pre_topk == k
    assert [r["count"] for r in ref["pre_topk_1"]] == [5, 5]
    c = T.BY_NAME["post_topk_one_below_survivors"]
    assert min(r["survivors"] for r in ref[c.name]) == c.post_topk + 1 and all(r["count"] == c.post_topk for r in ref[c.name])
    assert all(r["count"] == 1 for r in ref["post_topk_1"]) and all(r["survivors"] > 1 for r in ref["post_topk_1"])
    assert all(0 < r["count"] < 300 for r in ref["post_topk_1000_few_survivors"])
    assert all(r["count"] == 1024 for r in ref["post_topk_1024"])
    assert [T.BY_NAME[n].head_ld for n in ("head_ld_15", "head_ld_17", "head_ld_20", "head_ld_16_base_offset_1")] == [15, 17, 20, 16]
    for n in ("head_ld_17", "head_ld_20", "head_ld_16_base_offset_1"):
        assert all(np.abs(h[..., 15:]).min() > 1e37 for h in T.BY_NAME[n].heads), "padding columns must hold junk"
    # decode edges
    r = ref["decode_size_clamp"]
    w0 = (r[0]["boxes"][:5, 2] - r[0]["boxes"][:5, 0])
    h1 = (r[1]["boxes"][:5, 3] - r[1]["boxes"][:5, 1])
    assert np.allclose(w0, 125.0, atol=1e-4) and np.allclose(h1, 125.0, atol=1e-4), (w0, h1)      # 2 px x 1000 / 16, all five
    assert w0[1] < w0[0] and h1[1] < h1[0], "one float under the clamp must be a smaller box"
    assert [x["dropped"] for x in ref["decode_not_finite_deltas"]] == [dict(not_finite=8, empty=0), dict(not_finite=4, empty=0),
                                                                        dict(not_finite=4, empty=4)]
    assert [s for _, s in _rows(ref["decode_not_finite_deltas"][0])][:1] == [3.0], "every NaN row outranks the first ordinary one"
    ob = T.BY_NAME["decode_outside_and_borders"]
    assert [x["dropped"]["empty"] for x in ref[ob.name]] == [5, 4, 2]
    assert abs(min(x["margins"]["extent"] for x in ref[ob.name]) - 2.0 ** -9) < 1e-12
    assert abs(min(x["margins"]["empty"] for x in ref[ob.name]) - 2.0 ** -9) < 1e-12
    assert ob.img_h % ob.strides[0] and ob.img_w % ob.strides[0]
    # NMS
    for x in ref["nms_dense_clusters"]:
        assert int((x["src"][:, 0] == 0).sum()) == 5, "five clusters, one survivor each"
    ch = {0: ((62, 63, 64), (10, 11, 12)), 1: ((63, 64, 66), (126, 128, 129)), 2: ((62, 65, 66), (127, 128, 130))}
    cc = T.BY_NAME["nms_chain_across_words"]
    for n, x in enumerate(ref[cc.name]):
        order = np.argsort(-cc.heads[0][n, :, :, :3].reshape(-1).astype(np.float64), kind="stable")
        for ci, ranks in enumerate(ch[n]):
            for j, rk in enumerate(ranks):
                assert int(order[rk]) == ((6 + 10 * ci) * 20 + 10 + j) * 3 + j, "a chain row is not at its rank"
                assert _has(x, 0, 6 + 10 * ci, 10 + j, j) == (j != 1), ("chain", n, ci, j)       # A and C survive, B does not
    for x in ref["nms_invalid_row_suppresses_nothing"]:
        assert not _has(x, 0, 8, 8, 0) and _has(x, 0, 8, 9, 1) and not _has(x, 0, 8, 10, 2)
        assert x["dropped"] == dict(not_finite=1, empty=0)
    for c in T.CASES:
        if "rows_of_levels_0_1" in c.expect:
            assert [int((x["src"][:, 0] <= 1).sum()) for x in ref[c.name]] == [c.expect["rows_of_levels_0_1"]] * 2, c.name
    # levels and merge
    for x in ref["levels_do_not_interact"]:
        assert _rows(x)[:2] == [(0, 3.0), (1, 2.0)] and 1.0 not in [s for _, s in _rows(x)]
        assert (x["boxes"][0] == x["boxes"][1]).all()
    for x in ref["merge_ties"]:
        assert _rows(x)[:10] == T.BY_NAME["merge_ties"].expect["lead"]
        i = x["src"][6:9]
        flat = (i[:, 1] * 20 + i[:, 2]) * 3 + i[:, 3]
        assert (np.diff(flat) > 0).all(), "equal scores of one level: lower index first"
    z = ref["zero_survivors"]
    assert z[0]["count"] == 0 and not z[0]["boxes"].any() and not z[0]["scores"].any() and z[1]["count"] == 1000
    assert z[0]["dropped"]["not_finite"] > 0 and z[0]["dropped"]["empty"] > 0
    assert sum(n.startswith("random_") for n in T.NAMES) == 3


def _bar(r):
    """[count, 4]: the largest |coordinate - reference| allowed on every output row."""
    S = r["S"]
    return 4.0 * T.F32_VS_REF * ULP * np.stack([S[:, 0], S[:, 1], S[:, 0], S[:, 1]], axis=1)


def test_float32_decode_against_the_reference_is_the_recorded_figure():
    worst = (0.0, None)
    for c in T.CASES:
        for n, r in enumerate(T.reference(c)):
            k = r["count"]
            if k == 0:
                continue
            src = r["src"]
            got = np.zeros((k, 4))
            for lv in range(5):
                m = src[:, 0] == lv
                if not m.any():
                    continue
                hh, ww, aa = src[m, 1], src[m, 2], src[m, 3]
                d = c.heads[lv][n][hh, ww][:, 3:15].reshape(-1, 3, 4)[np.arange(int(m.sum())), aa]
                b = REF.decode_f32(d, hh, ww, aa, c.cell[lv], c.strides[lv])
                got[m] = REF.clip(b.astype(np.float64), c.img_h, c.img_w)
            S = np.stack([r["S"][:, 0], r["S"][:, 1]] * 2, axis=1)
            err = np.abs(got - r["boxes"][:k]) / (ULP * S)
            i = np.unravel_index(int(err.argmax()), err.shape)
            if err[i] > worst[0]:
                worst = (float(err[i]), (c.name, n, int(i[0]), int(i[1])))
    print(f"largest |float32 decode - reference| = {worst[0]:.3f} x 2^-24 S at {worst[1]}; record {T.F32_VS_REF}, GPU bar {4 * T.F32_VS_REF} x 2^-24 S")
    # (numpy's float32 exp may differ by an ulp from one CPU to the next: a quarter more)
    assert worst[0] <= 1.25 * T.F32_VS_REF, worst
    assert worst[0] >= T.F32_VS_REF / 2, ("the record is stale: measure again", worst)


def _anchors(R, c, lv, h, w, restate=False):
    """The level's anchors [h w 3, 4] float32 as ``grid_anchors`` builds them, for the case's own cell table."""
    st = int(c.strides[lv])
    if not restate and np.array_equal(c.cell, T.cell_table()):
        return R.grid_anchors(h, w, st, float(T.SIZES[lv]))
    sx = torch.arange(0, w * st, step=st, dtype=torch.float32)
    sy = torch.arange(0, h * st, step=st, dtype=torch.float32)
    yy, xx = torch.meshgrid(sy, sx, indexing="ij")
    shifts = torch.stack((xx.reshape(-1), yy.reshape(-1), xx.reshape(-1), yy.reshape(-1)), dim=1)
    return (shifts.view(-1, 1, 4) + torch.from_numpy(c.cell[lv]).view(1, -1, 4)).reshape(-1, 4)


def _oracle(R, c, n):
    """One image through the oracle's blocks, assembled as ``oracle.maskrcnn_ref.rpn_forward`` assembles them."""
    all_boxes, all_scores, all_lvl, all_idx = [], [], [], []
    for lv, head in enumerate(c.heads):
        h, w = head.shape[1], head.shape[2]
        logits_f = torch.from_numpy(np.ascontiguousarray(head[n, :, :, :3]).reshape(-1))
        deltas_f = torch.from_numpy(np.ascontiguousarray(head[n, :, :, 3:15]).reshape(-1, 4))
        anchors = _anchors(R, c, lv, h, w)
        k = min(logits_f.numel(), c.pre_topk)
        order = torch.sort(logits_f, descending=True, stable=True)[1][:k]
        all_boxes.append(R.apply_deltas(deltas_f[order], anchors[order], (1.0, 1.0, 1.0, 1.0)))
        all_scores.append(logits_f[order])
        all_lvl.append(torch.full((k,), lv, dtype=torch.int64))
        all_idx.append(order)
    boxes, scores, lvl, idx = torch.cat(all_boxes), torch.cat(all_scores), torch.cat(all_lvl), torch.cat(all_idx)
    valid = torch.isfinite(boxes).all(dim=1) & torch.isfinite(scores)
    boxes, scores, lvl, idx = boxes[valid].clone(), scores[valid], lvl[valid], idx[valid]
    boxes[:, 0].clamp_(min=0, max=c.img_w)
    boxes[:, 1].clamp_(min=0, max=c.img_h)
    boxes[:, 2].clamp_(min=0, max=c.img_w)
    boxes[:, 3].clamp_(min=0, max=c.img_h)
    nonempty = ((boxes[:, 2] - boxes[:, 0]) > 0) & ((boxes[:, 3] - boxes[:, 1]) > 0)
    boxes, scores, lvl, idx = boxes[nonempty], scores[nonempty], lvl[nonempty], idx[nonempty]
    if boxes.shape[0] == 0:
        keep = torch.zeros((0,), dtype=torch.int64)
    else:
        keep = R.batched_nms(boxes, scores, lvl, c.nms_thresh)[:c.post_topk]
    wd = np.array([c.heads[int(l)].shape[2] for l in lvl[keep]], dtype=np.int64)
    i = idx[keep].numpy()
    src = np.stack([lvl[keep].numpy(), (i // 3) // np.maximum(wd, 1), (i // 3) % np.maximum(wd, 1), i % 3], axis=1) if len(i) else np.zeros((0, 4), dtype=np.int64)
    return boxes[keep].numpy(), scores[keep].numpy(), src


def test_reference_agrees_with_the_oracle_blocks_on_every_case():
    from oracle import maskrcnn_ref as R

    c0 = T.BY_NAME["select_smooth"]
    for lv, (h, w) in enumerate(T.SHAPES):                                  # the restated anchor grid is grid_anchors itself
        assert torch.equal(_anchors(R, c0, lv, h, w, restate=True), R.grid_anchors(h, w, T.STRIDES[lv], float(T.SIZES[lv])))
    assert abs(R.SCALE_CLAMP - REF.SCALE_CLAMP) == 0.0
    bad, worst = [], (0.0, None)
    for c in T.CASES:
        for n, r in enumerate(T.reference(c)):
            ob, os_, osrc = _oracle(R, c, n)
            k = r["count"]
            if len(os_) != k:
                bad.append((c.name, n, "count", len(os_), k))
                continue
            if not np.array_equal(osrc, r["src"]):
                bad.append((c.name, n, "kept rows or their order", int((osrc != r["src"]).any(axis=1).argmax())))
                continue
            if not np.array_equal(os_.view(np.uint32), r["scores"][:k].view(np.uint32)):
                bad.append((c.name, n, "scores"))
            if k:
                rel = np.abs(ob.astype(np.float64) - r["boxes"][:k]) / _bar(r)
                if rel.max() > worst[0]:
                    worst = (float(rel.max()), (c.name, n))
                if rel.max() > 1.0:
                    bad.append((c.name, n, "boxes", float(rel.max())))
    print(f"oracle against reference: same rows, order and counts on {len(T.CASES)} cases; worst box difference {worst[0]:.3f} of the bar at {worst[1]}")
    assert not bad, bad


# the cases each mutant is tried on: the ones built for the rule it breaks (all seven mutants run on all of them)
MUTANT_CASES = ("select_quantised", "select_all_equal", "merge_ties", "nms_thresh_exactly_0.5_at", "nms_thresh_exactly_0.75_at",
                "levels_do_not_interact", "decode_not_finite_deltas", "zero_survivors", "decode_size_clamp", "pre_topk_1", "pre_topk_63",
                "pre_topk_64", "pre_topk_65", "nms_chain_across_words")


def test_the_reference_notices_each_of_seven_mistakes():
    caught = {m: [] for m in REF.MUTANTS}
    only_record = {m: True for m in REF.MUTANTS}
    for name in MUTANT_CASES:
        c = T.BY_NAME[name]
        ref = T.reference(c)
        for m in REF.MUTANTS:
            got = REF.proposals(c.heads, c.cell, c.strides, c.img_h, c.img_w, c.pre_topk, c.post_topk, c.nms_thresh, mutant=m)
            rows = any(g["count"] != r["count"] or not np.array_equal(g["src"], r["src"]) or not np.array_equal(g["boxes"], r["boxes"])
                       or not np.array_equal(g["scores"].view(np.uint32), r["scores"].view(np.uint32)) for g, r in zip(got, ref))
            record = any(g["dropped"] != r["dropped"] for g, r in zip(got, ref))
            if rows or record:
                caught[m].append(name)
                only_record[m] = only_record[m] and not rows
    for m in REF.MUTANTS:
        print(f"mutant {m:26s} caught by: {', '.join(caught[m]) or 'NOTHING'}" + ("   (in the record of dropped rows only)" if caught[m] and only_record[m] else ""))
    assert all(caught.values()), {m: v for m, v in caught.items() if not v}
    # Clipping before the finiteness test cannot change an OUTPUT row, in any implementation: a clamped size is finite, so a
    # non-finite centre makes both coordinates of its axis the same infinity (clipped onto ONE plane: extent 0, dropped as
    # empty) or NaN (stays NaN).  The mutant only books the row under another reason, and that is where it is caught.
    assert only_record["clip_before_finite_test"]
    assert not any(only_record[m] for m in REF.MUTANTS if m != "clip_before_finite_test")
