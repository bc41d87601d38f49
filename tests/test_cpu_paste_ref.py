"""The mask paste's reference and case table, checked without a GPU.

  * the table holds what it says: the frame layouts, every slot's validity, the column path each window of the wide frame
    selects (both paths, and the windows of exactly 2048 and 2049 columns), an exact family with pixels at exactly 0.5;
  * the reference (``paste_ref.py``: f32 box contract, f64 sampling as two tap-weight matrices) agrees with the oracle
    (``oracle.maskrcnn_ref.paste_masks``: torch f32 ``grid_sample``) over the whole table: boxes bit-equal, sampled
    probabilities within the tie band ``TAU``, decisions equal outside it, and on the exact family everything bit-equal;
  * ambiguous pixels are at most ``MAX_AMBIGUOUS_SHARE`` of the table's window pixels, and every valid slot has decided
    pixels of both values, so a paste that fills or empties a window cannot pass.
"""
import numpy as np
import pytest
import torch

import paste_cases as T
import paste_ref as REF


def test_the_frames_cover_the_row_and_word_layouts():
    frames = [c.frame for c in T.CASES]
    assert {32, 33, 77, 128, 333}.issubset({f.out_w for f in frames})
    wide = [f for f in frames if f.out_w > T.PASTE_COLS]
    assert wide and all(f.out_h <= 48 for f in wide)
    assert any(f.out_h % T.PASTE_ROWS == 0 for f in frames) and any(f.out_h % T.PASTE_ROWS for f in frames)
    assert any(f.wpr % 4 == 0 and f.out_h % T.PASTE_ROWS for f in frames), "16-byte zero rows with a short last chunk"
    assert any(f.wpr % 4 == 0 for f in frames) and any(f.wpr % 4 for f in frames)
    assert any(f.out_w % 32 == 0 for f in frames) and any(f.out_w % 32 for f in frames)
    ratios = [(f.out_w / f.img_w, f.out_h / f.img_h) for f in frames if f.rescales]
    assert any(rx < 1 and ry < 1 for rx, ry in ratios) and any(rx > 1 and ry > 1 for rx, ry in ratios)
    assert all(rx != ry for rx, ry in ratios)
    # counts: 0, 1 and D, and images of one call with different counts
    counts = [c.counts for c in T.CASES]
    assert any(0 in c for c in counts) and any(1 in c for c in counts) and any(cs.D in cs.counts for cs in T.CASES)
    assert any(len(set(c)) > 1 for c in counts)
    assert all(0 <= k <= c.D for c in T.CASES for k in c.counts)
    assert all(len(img) == c.D for c in T.CASES for img in c.slots)
    assert all(0 <= s.cls < c.K for c in T.CASES for img in c.slots for s in img)
    for frame, names in T.INCREMENTAL.items():
        cs = [T.BY_NAME[n] for n in names]
        assert len(cs) == 3 and len({(c.frame, c.N, c.D) for c in cs}) == 1 and cs[0].frame.name == frame
    inc = [T.FRAMES[k] for k in T.INCREMENTAL]
    assert any(f.wpr % 4 and f.out_h % T.PASTE_ROWS for f in inc) and any(f.out_w > T.PASTE_COLS for f in inc)


def test_every_slot_meets_its_expectation():
    bad, paths, ncols = [], set(), set()
    for c in T.CASES:
        ref = T.reference(c)
        for n, i, s in c.used():
            e = s.expect
            if "valid" in e and bool(ref.valid[n, i]) != e["valid"]:
                bad.append((c.name, s.name, "valid", bool(ref.valid[n, i])))
            if not ref.valid[n, i]:
                if (ref.hint[n, i] != -1).any() or (n, i) in ref.prob:
                    bad.append((c.name, s.name, "an invalid slot has a window"))
                continue
            path, ncol = T.column_path(ref.hint[n, i]), int(ref.hint[n, i, 3] - ref.hint[n, i, 1] + 1)
            if c.frame.out_w > T.PASTE_COLS:
                paths.add(path)
                ncols.add(ncol)
            elif path != "table":
                bad.append((c.name, s.name, "path", path))
            if e.get("path", path) != path or e.get("ncol", ncol) != ncol:
                bad.append((c.name, s.name, "path", path, ncol))
        for n in range(c.N):
            assert not ref.valid[n, c.counts[n]:].any() and not ref.out_boxes[n, c.counts[n]:].any()
            assert (ref.hint[n, c.counts[n]:] == -1).all()
    assert not bad, bad
    assert paths == {"table", "pixel"}
    assert {T.PASTE_COLS, T.PASTE_COLS + 1, T.FRAMES["wide"].out_w}.issubset(ncols) and min(ncols) < T.PASTE_COLS
    # every incremental sequence has slots that were pasted in one round and are invalid or unused in the next, and the reverse
    for names in T.INCREMENTAL.values():
        v = [T.reference(T.BY_NAME[n]).valid for n in names]
        gone = sum(int((v[r - 1] & ~v[r]).sum()) for r in (1, 2))
        back = sum(int((~v[r - 1] & v[r]).sum()) for r in (1, 2))
        assert gone >= 5 and back >= 5, (names, gone, back)


def test_out_boxes_are_the_oracles_f32_boxes_bit_for_bit():
    """The oracle's ``predict`` scales with a Python float on f32 tensors, then clamps: the same numbers, bit for bit."""
    for c in T.CASES:
        f = c.frame
        ob, valid = REF.out_boxes(c.det_boxes(), f.img_h, f.img_w, f.out_h, f.out_w)
        t = torch.from_numpy(c.det_boxes()).reshape(-1, 4).clone()
        t[:, 0::2] *= f.out_w / f.img_w
        t[:, 1::2] *= f.out_h / f.img_h
        t[:, 0].clamp_(min=0, max=f.out_w)
        t[:, 1].clamp_(min=0, max=f.out_h)
        t[:, 2].clamp_(min=0, max=f.out_w)
        t[:, 3].clamp_(min=0, max=f.out_h)
        nonempty = ((t[:, 2] - t[:, 0]) > 0) & ((t[:, 3] - t[:, 1]) > 0)
        assert ob.dtype == np.float32 and np.array_equal(ob.reshape(-1, 4).view(np.uint32), t.numpy().view(np.uint32)), c.name
        assert np.array_equal(valid.reshape(-1), nonempty.numpy()), c.name


def test_the_reference_agrees_with_the_oracle_paste():
    from oracle import maskrcnn_ref as R

    worst = (0.0, None)
    for c in T.CASES:
        ref, f = T.reference(c), c.frame
        masks = c.masks()
        for n in range(c.N):
            idx = np.nonzero(ref.valid[n])[0]
            if len(idx) == 0:
                continue
            args = (torch.from_numpy(masks[n, idx]), torch.from_numpy(ref.out_boxes[n, idx].copy()), f.out_h, f.out_w)
            soft = R.paste_masks(*args, soft=True).numpy()
            hard = R.paste_masks(*args).numpy()
            for k, i in enumerate(idx):
                name = (c.name, n, c.slots[n][i].name)
                y0, x0, y1, x1 = ref.hint[n, i]
                p = ref.prob[(n, int(i))]
                inside = np.zeros((f.out_h, f.out_w), dtype=bool)
                inside[y0:y1 + 1, x0:x1 + 1] = True
                assert not hard[k][~inside].any() and not soft[k][~inside].any(), name
                s, h = soft[k, y0:y1 + 1, x0:x1 + 1], hard[k, y0:y1 + 1, x0:x1 + 1]
                if c.exact:
                    assert np.array_equal(s.astype(np.float64), p), name
                    assert np.array_equal(h, p >= 0.5), name
                    continue
                err = float(np.abs(s.astype(np.float64) - p).max())
                if err > worst[0]:
                    worst = (err, name)
                assert err <= T.TAU, (name, err)
                dec = T.decided(c, p)
                assert np.array_equal(h[dec], (p >= 0.5)[dec]), (name, int((h != (p >= 0.5))[dec].sum()))
    print(f"largest |oracle f32 - reference f64| over the table: {worst[0]:.3e} at {worst[1]} (tie band {T.TAU:.3e})")
    assert worst[0] <= T.TAU / 4, worst        # the band leaves room for a second f32 implementation


def test_the_exact_family_is_exact_and_has_pixels_at_one_half():
    cs = [c for c in T.CASES if c.exact]
    assert cs
    ties = 0
    for c in cs:
        ref, f = T.reference(c), c.frame
        assert not f.rescales
        assert np.array_equal(ref.out_boxes[:, : c.counts[0]], c.det_boxes()[:, : c.counts[0]]), "the clip changed an exact box"
        for n, i, s in c.used():
            x0, y0, x1, y1 = s.box
            assert (x1 - x0) in (16, 32, 64, 128) and (y1 - y0) in (16, 32, 64, 128), s.name
            assert all(float(v * 4).is_integer() for v in s.box), s.name
            assert np.array_equal(s.mask * 4, np.round(s.mask * 4)), s.name
            p = ref.prob[(n, i)]
            assert np.array_equal(p, p.astype(np.float32).astype(np.float64)), s.name
            assert np.array_equal(p * 2.0 ** 16, np.round(p * 2.0 ** 16)), s.name
            ties += int((p == 0.5).sum())
        assert any((s.mask == 1).all() for _, _, s in c.used())
    print(f"exact family: {ties} pixels at exactly 0.5")
    assert ties >= 100, ties


def test_ambiguous_pixels_are_few_and_every_window_has_both_values():
    amb = total = needed = slots = 0
    one_sided = []
    for c in T.CASES:
        ref = T.reference(c)
        for n, i, s in c.used():
            if not ref.valid[n, i]:
                continue
            p = ref.prob[(n, i)]
            dec = T.decided(c, p)
            slots += 1
            if not c.exact:
                amb += int((~dec).sum())
                total += p.size
            needed += T.needs_both_values(s, ref.out_boxes[n, i])
            if T.needs_both_values(s, ref.out_boxes[n, i]) and not (((p >= 0.5) & dec).any() and ((p < 0.5) & dec).any()):
                one_sided.append((c.name, n, s.name))
    print(f"ambiguous pixels: {amb} of {total} window pixels = {100.0 * amb / total:.4f} %")
    assert amb <= T.MAX_AMBIGUOUS_SHARE * total, (amb, total)
    assert not one_sided, one_sided
    print(f"{needed} of {slots} valid slots are named or hold three pixel centres per axis")
    assert needed >= 0.8 * slots


def test_the_blocked_layout_helper_puts_each_cell_in_its_row_and_column():
    rng = np.random.default_rng(3)
    n, K = 3, 5
    masks = rng.random((n, 28, 28)).astype(np.float32)
    classes = np.array([4, 0, 2])
    b = REF.blocked_mask_prob(masks, classes, K)
    ld = 8
    assert b.shape == (n * 196 * 4, ld) and b.dtype == np.float32
    for inst in range(n):
        for y in (0, 1, 13, 27):
            for x in (0, 1, 14, 27):
                row = (inst * 196 + (y >> 1) * 14 + (x >> 1)) * 4 + (y & 1) * 2 + (x & 1)
                assert b[row, classes[inst]] == masks[inst, y, x]
                others = [k for k in range(K) if k != classes[inst]]
                assert (b[row, others] == -1.0).all() and (b[row, K:] == 7.0).all()


@pytest.mark.parametrize("W", [1, 31, 32, 33, 77, 128])
def test_pack_and_unpack_bits_are_inverse(W):
    rng = np.random.default_rng(W)
    dense = rng.random((2, 5, W)) < 0.5
    words = REF.pack_bits(dense)
    assert words.shape == (2, 5, (W + 31) // 32) and words.dtype == np.uint32
    for x in range(W):
        assert np.array_equal((words[..., x >> 5] >> np.uint32(x & 31)) & 1, dense[..., x])
    back = REF.unpack_bits(words, W)
    assert np.array_equal(back[..., :W], dense) and not back[..., W:].any()
