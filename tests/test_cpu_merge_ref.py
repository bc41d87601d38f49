"""The tile-merge references and case tables (``merge_ref.py``, ``merge_cases.py``), checked without a GPU -- and the one host
function of the placement that loses pixels silently when it is too tight, ``cropset.rooms_of_placed_tiles``.

  * the nearest rule: three independent writings (the reference's scalar loop, ``oracle.postproc_ref.resize_nearest``,
    ``cropset.nearest_index``) agree on every size pair of the table; each of the three wrong writings differs at every
    tell-tale pair, and in every tell-tale placement case each would change a placed pixel;
  * ``rooms_of_placed_tiles`` over the whole placement table, with tight and grown source boxes: the room contains the placed
    mask, is -1 exactly when the box can reach no pixel of the frame, equals the tight box for the identity resize;
  * the overlap reference: outputs of a segment disjoint, their union the union of the inputs, each inside its input,
    idempotent; column counts sum to the areas; ``pack`` / ``unpack`` round-trip;
  * the table conditions: chains over one pixel in the overlap cases, the size caps, what the geometry list promises.
"""
import numpy as np
import pytest

import merge_cases as T
import merge_ref as REF


# ------------------------------------------------------------------------------------------------------------ index rule
def test_nearest_rule_in_three_writings():
    from deepemia_amd.cropset import nearest_index
    from oracle import postproc_ref as P

    pairs = T.place_size_pairs()
    assert len(pairs) > 30
    for n_dst, n_src in pairs:
        want = REF.nearest_rule(n_dst, n_src)
        assert want.shape == (n_dst,) and want[0] == 0 and (np.diff(want) >= 0).all() and want[-1] <= n_src - 1
        assert np.array_equal(nearest_index(n_dst, n_src), want), (n_dst, n_src)
        ramp = np.arange(n_src, dtype=np.int64)
        assert np.array_equal(P.resize_nearest(np.repeat(ramp[:, None], 2, axis=1), n_dst, 2)[:, 0], want), (n_dst, n_src)
        assert np.array_equal(P.resize_nearest(np.repeat(ramp[None, :], 2, axis=0), 2, n_dst)[0], want), (n_dst, n_src)


@pytest.mark.parametrize("pair", T.TELLTALE, ids=lambda p: f"{p[1]}_to_{p[0]}")
def test_every_wrong_rule_differs_at_a_telltale_pair(pair):
    want = REF.nearest_rule(*pair)
    for name, rule in REF.WRONG_RULES.items():
        got = rule(*pair)
        assert got.shape == want.shape and (got != want).any(), (pair, name)
        assert np.abs(got - want).max() == 1, (pair, name)             # a neighbouring source pixel: what a checkerboard shows


def test_the_wrong_rules_pass_at_the_sizes_the_suite_had_before():
    """Why the table exists: at 128 -> 64, 64 -> 64 and 96 -> 64 every wrong rule gives the right answer."""
    for pair in ((64, 128), (64, 64), (64, 96)):
        for rule in REF.WRONG_RULES.values():
            assert np.array_equal(rule(*pair), REF.nearest_rule(*pair))
    # the multi-scale path at s = 0.7 does differ (integer and f32 forms)
    assert REF.rule_integer(100, 70)[90] != REF.nearest_rule(100, 70)[90]
    assert int((REF.rule_integer(200, 140) != REF.nearest_rule(200, 140)).sum()) == 3


def test_the_placement_table_holds_what_it_says():
    cases = T.PLACE_CASES
    assert all(c.frame[0] <= T.MAX_FRAME[0] and c.frame[1] <= T.MAX_FRAME[1] and c.T <= T.MAX_T for c in cases)
    assert all(len(c.kinds) == c.T for c in cases)
    assert any(c.T == 0 for c in cases) and any(c.frame[0] == 1 for c in cases)
    assert any(c.frame[1] % 32 for c in cases) and any(c.frame[1] % 32 == 0 for c in cases)
    assert any(c.src[1] % 32 for c in cases) and any(c.src[1] % 32 == 0 for c in cases)
    have = {(c.src, c.tile) for c in cases}
    assert {((64, 64), (64, 64)), ((128, 128), (64, 64)), ((96, 96), (64, 64)), ((300, 300), (200, 200))} <= have
    for h, w in T.MULTISCALE_FRAMES:
        for s in T.SCALES:
            assert ((int(h * s), int(w * s)), (h, w)) in have
    assert ((70, 91), (100, 130)) in have
    for d, s in T.TELLTALE:
        assert ((s, s), (d, d)) in have
    mixed = [c for c in cases if c.telltale and c.tile[0] / c.src[0] != c.tile[1] / c.src[1]]
    assert any(c.tile[0] > c.src[0] and c.tile[1] < c.src[1] for c in mixed) and any(c.tile[0] < c.src[0] and c.tile[1] > c.src[1] for c in mixed)
    for c in cases:
        if c.telltale:
            assert all(p in T.TELLTALE for p in c.size_pairs()), c.name
    # the geometry list, in a frame with a partly used last word and in one without
    for W in (77, 96):
        geo = [c for c in cases if c.name.startswith("geometry_") and c.frame[1] == W]
        assert {k for c in geo for k in c.kinds} == {"random", "ones", "checker"}
        H = geo[0].frame[0]
        th, tw = geo[0].tile
        offs = {o for c in geo for o in c.offsets}
        xs = {o[0] for o in offs}
        assert {0, 1, 31, 32, 33, 63} <= xs
        assert any(0 <= x < W < x + tw and 0 <= y and y + th <= H for x, y in offs)          # across the right edge only
        assert any(0 <= y < H < y + th and 0 <= x and x + tw <= W for x, y in offs)          # across the bottom edge only
        assert any(x < W < x + tw and y < H < y + th for x, y in offs)                       # across both
        assert any(x + tw == W for x, y in offs) and any(y + th == H for x, y in offs)       # ending exactly at the last column / row
        assert any(x >= W for x, y in offs) and any(y >= H for x, y in offs) and any(x <= -tw for x, y in offs)
        assert any(x < 0 and y < 0 and x + tw > 0 and y + th > 0 for x, y in offs)           # first rows and columns cut
        assert any(x == W - 1 for x, y in offs)                                              # one column, in the last word
    kinds = {k for c in cases for k in c.kinds}
    assert kinds == set(T.KINDS)


@pytest.mark.parametrize("name", [c.name for c in T.PLACE_CASES if c.telltale])
def test_every_wrong_rule_changes_a_placed_pixel_of_a_telltale_case(name):
    """The tell-tale indices are visible: they lie in the part of the tile that lands in the frame, at pixels where the mask
    differs between the two candidate source pixels."""
    diff = T.wrong_rule_pixels(T.PLACE_BY_NAME[name])
    assert set(diff) == set(REF.WRONG_RULES) and all(v > 0 for v in diff.values()), (name, diff)


def test_wrong_rule_pixels_over_the_table():
    """The figure the table carries, for the record: per wrong rule, the cases it would fail and the pixels that differ."""
    per_rule = {k: [0, 0] for k in REF.WRONG_RULES}
    for c in T.PLACE_CASES:
        for k, v in T.wrong_rule_pixels(c).items():
            per_rule[k][0] += v > 0
            per_rule[k][1] += v
    print("wrong rule -> (cases that would fail, pixels that would differ):", per_rule)
    n_tell = sum(c.telltale for c in T.PLACE_CASES)
    assert all(v[0] >= n_tell for v in per_rule.values())
    # the pipeline's own multi-scale sizes at s = 0.7 catch the integer and the f32 form
    for k in ("integer", "f32"):
        assert T.wrong_rule_pixels(T.PLACE_BY_NAME["multiscale_100x130_s0.7"])[k] > 0


def test_all_ones_places_the_clipped_rectangle_and_padding_never_shows():
    for c in T.PLACE_CASES:
        H, W = c.frame
        for t, kind in enumerate(c.kinds):
            if kind != "ones":
                continue
            xo, yo = c.offsets[t]
            want = np.zeros((H, W), dtype=bool)
            want[max(yo, 0):max(min(yo + c.tile[0], H), 0), max(xo, 0):max(min(xo + c.tile[1], W), 0)] = True
            assert np.array_equal(T.placed(c)[t], want), (c.name, t)
    c = T.PLACE_BY_NAME["geometry_a_w77_random"]
    words = T.packed_sources(c)
    dense, pad = REF.unpack(words, c.src[1])
    assert np.array_equal(dense, T.sources(c)) and pad.all() and pad.shape[-1] == 64 - 52


# ------------------------------------------------------------------------------------------------ rooms_of_placed_tiles
def _filled(boxes, hw):
    out = np.zeros((len(boxes),) + tuple(hw), dtype=bool)
    for i, (y0, x0, y1, x1) in enumerate(boxes):
        if y0 >= 0:
            out[i, y0:y1 + 1, x0:x1 + 1] = True
    return out


@pytest.mark.parametrize("grown", [False, True], ids=["tight_boxes", "grown_boxes"])
@pytest.mark.parametrize("name", [c.name for c in T.PLACE_CASES])
def test_rooms_of_placed_tiles(name, grown):
    from deepemia_amd.cropset import rooms_of_placed_tiles

    c = T.PLACE_BY_NAME[name]
    H, W = c.frame
    boxes = T.source_boxes(c)
    if grown:
        boxes = T.grow_boxes(boxes, c.src, by=(2, 3, 1, 5))
    rooms = rooms_of_placed_tiles(boxes, c.src, c.tile, c.xo, c.yo, c.frame)
    assert rooms.shape == (c.T, 4) and rooms.dtype == np.int32
    reach = _filled(boxes, c.src)                      # every source pixel the box allows
    identity = c.src == c.tile
    for t in range(c.T):
        room = rooms[t].tolist()
        xo, yo = c.offsets[t]
        area, box = REF.area_bbox(T.placed(c)[t])
        can_area, can_box = REF.area_bbox(REF.place(reach[t], c.tile[0], c.tile[1], xo, yo, H, W))
        what = (name, t, c.kinds[t], c.offsets[t], boxes[t].tolist(), room)
        # -1 exactly when no pixel of the frame takes its value from inside the box (an empty source; a tile outside the frame;
        # a box the resize skips; a box whose part of the tile is clipped away)
        assert (room[0] < 0) == (can_area == 0), what
        if room[0] < 0:
            assert room == [-1, -1, -1, -1] and area == 0, what
            continue
        assert 0 <= room[0] <= room[2] <= H - 1 and 0 <= room[1] <= room[3] <= W - 1, what
        # the room is the box of everything the source box can reach -- so it contains the placed mask, whatever the mask
        assert room == can_box, what
        if area:
            assert room[0] <= box[0] and room[1] <= box[1] and room[2] >= box[2] and room[3] >= box[3], what
        if identity and not grown:
            assert room == box, what


def test_rooms_see_masks_that_are_clipped_or_skipped_away():
    """Empty placed masks of non-empty sources occur in the table: clipped away by the frame, and lost by a shrinking resize."""
    from deepemia_amd.cropset import rooms_of_placed_tiles

    clipped = skipped = 0
    for c in T.PLACE_CASES:
        boxes = T.source_boxes(c)
        rooms = rooms_of_placed_tiles(boxes, c.src, c.tile, c.xo, c.yo, c.frame)
        for t in range(c.T):
            if boxes[t, 0] >= 0 and not T.placed(c)[t].any():
                inside = all(0 <= o and o + n <= f for o, n, f in zip((c.offsets[t][1], c.offsets[t][0]), c.tile, c.frame))
                # (a checkerboard halved exactly is empty too, with a full room: a room is an upper bound)
                skipped += inside and rooms[t, 0] < 0
                clipped += not inside
    assert clipped >= 10 and skipped >= 1, (clipped, skipped)
    # a source pixel in a row and a column that 148 -> 40 skips: nothing of it is placed, and the room says so
    assert 2 not in REF.nearest_rule(40, 148)
    room = rooms_of_placed_tiles(np.array([[2, 2, 2, 2]]), (148, 148), (40, 40), [0], [0], (40, 40))
    assert room.tolist() == [[-1, -1, -1, -1]]
    room = rooms_of_placed_tiles(np.array([[2, 2, 3, 3]]), (148, 148), (40, 40), [5], [7], (60, 60))
    assert room.tolist() == [[8, 6, 8, 6]] and REF.nearest_rule(40, 148)[1] == 3


# -------------------------------------------------------------------------------------------------------------- overlap
@pytest.mark.parametrize("name", [c.name for c in T.OVERLAP_CASES])
def test_overlap_reference_properties(name):
    c = T.OVERLAP_BY_NAME[name]
    masks, seg, out = T.overlap_masks(c), c.seg(), T.overlap_want(c)
    assert masks.shape == (c.M,) + c.frame and out.shape == masks.shape
    assert seg is None or ((np.diff(seg) >= 0).all() and len(seg) == c.M and len(set(seg.tolist())) == len(c.lengths))
    assert not (out & ~masks).any()                                              # each output inside its input
    ids = np.zeros(c.M, dtype=np.int64) if seg is None else seg
    for s in np.unique(ids):
        sel = ids == s
        assert out[sel].sum(axis=0).max() <= 1                                   # pairwise disjoint
        assert np.array_equal(out[sel].any(axis=0), masks[sel].any(axis=0))      # same union
    assert np.array_equal(REF.overlap_prefix(out, seg), out)                     # idempotent
    if c.full_first is not None:
        s = c.starts()[c.full_first]
        assert masks[s].all() and out[s].all() and not out[s + 1:s + c.lengths[c.full_first]].any()


def test_masks_more_than_a_chunk_apart_own_pixels_alone():
    """What makes the box kernel's later chunks visible: blobs are so dense that a mask 257 places back is almost never the
    ONLY earlier owner of a pixel -- some mask of the nearest 256 has it too, and a kernel that stopped after its first chunk
    would still give the right answer.  The planted pairs own their block of the quiet strip alone."""
    distances = {}
    for c in T.OVERLAP_CASES:
        masks, out = T.overlap_masks(c), T.overlap_want(c)
        H = c.frame[0]
        strip = slice(H - T.QUIET_ROWS, H)
        for k, (s, n) in enumerate(zip(c.starts(), c.lengths)):
            for h, m, x0 in T.far_pairs(int(s), int(n)):
                assert s <= h < m < s + n
                distances.setdefault(c.name, set()).add(m - h)
                block = (strip, slice(x0, x0 + 10))
                owners = [j for j in range(s, s + n) if masks[j][block].any()]
                want_owners = [h, m] if c.full_first != k else [s, h, m]
                assert owners == want_owners, (c.name, h, m, owners)
                assert masks[h][block][:, :9].all() and masks[m][block].all()
                if c.full_first == k:
                    assert not out[h][block].any() and not out[m][block].any()
                else:
                    assert out[h][block][:, :9].all()
                    assert not out[m][block][:, :9].any() and out[m][block][:, 9].all()         # lost to h alone; its own column kept
    assert distances["one_of_300"] == {256, 257} and distances["no_seg_270"] == {256, 257}
    assert distances["start_inside_a_chunk"] == {256, 257, 512, 513}
    assert distances["around_256"] == {256} and distances["full_frame_first_of_270"] == {256, 257}
    assert any(x0 < 32 < x0 + 9 for _, x0 in T.FAR)


def test_the_overlap_table_holds_what_it_says():
    lengths = [c.lengths for c in T.OVERLAP_CASES]
    for want in ((10, 10, 10, 10), (300,), (3, 300, 1, 530, 40), (256, 257, 255), (1,)):
        assert want in lengths
    assert any(not c.use_seg and c.M == 270 for c in T.OVERLAP_CASES)
    assert all(c.frame in ((40, 70), (33, 64)) for c in T.OVERLAP_CASES) and max(c.M for c in T.OVERLAP_CASES) <= 900
    for c in T.OVERLAP_CASES:
        masks, out = T.overlap_masks(c), T.overlap_want(c)
        if max(c.lengths) >= T.CHAIN_MIN_SEGMENT:
            share = T.chain_share(c)
            print(f"{c.name}: {share:.2f} of the masks lose a pixel that two or more earlier masks own")
            assert share >= 0.1, (c.name, share)
            tight = T.tight_boxes(masks)
            assert (tight[:, 0] < 0).any()                                       # empty inputs in the middle of segments
            assert (masks.any(axis=(1, 2)) & ~out.any(axis=(1, 2))).any()        # identical / covered masks come out empty
            # two masks that touch at a word boundary and do not overlap
            s = next(int(s) for s, n in zip(c.starts(), c.lengths) if n >= 10)
            a, b = masks[s + 3], masks[s + 4]
            assert a[:, 31].any() and b[:, 32].any() and not (a & b).any() and not a[:, 32:].any() and not b[:, :32].any()
        for mode in ("tight", "grown"):
            boxes = T.overlap_boxes(c, mode)
            tight = T.tight_boxes(masks)
            ok = tight[:, 0] >= 0
            assert (boxes[~ok] == -1).all()
            assert (boxes[ok, :2] <= tight[ok, :2]).all() and (boxes[ok, 2:] >= tight[ok, 2:]).all()
            assert (boxes[ok, :2] >= 0).all() and (boxes[ok, 2] <= c.frame[0] - 1).all() and (boxes[ok, 3] <= c.frame[1] - 1).all()
            if mode == "grown" and c.M > 5:
                assert (boxes != tight).any()
        assert T.overlap_boxes(c, "none") is None


# -------------------------------------------------------------------------------------------------------- column counts
@pytest.mark.parametrize("name", [c.name for c in T.COUNT_CASES])
def test_column_count_reference_and_table(name):
    c = T.COUNT_BY_NAME[name]
    masks, seg = T.count_inputs(c)
    H, W = c.frame
    counts = REF.column_counts(masks, seg, c.n_seg)
    assert counts.shape == (c.n_seg, W) and counts.dtype == np.int64
    areas = np.array([REF.area_bbox(m)[0] for m in masks])
    ids = np.zeros(len(masks), dtype=np.int64) if seg is None else seg
    for s in range(c.n_seg):
        assert counts[s].sum() == areas[ids == s].sum()
    assert len(masks) <= 65535
    boxes, tight = T.count_boxes(c), T.tight_boxes(masks)
    ok = tight[:, 0] >= 0
    assert (~ok).sum() >= 2 and (boxes[~ok] == -1).all()
    assert (boxes[ok, :2] <= tight[ok, :2]).all() and (boxes[ok, 2:] >= tight[ok, 2:]).all()
    assert (boxes[ok, :2] >= 0).all() and (boxes[ok, 2] <= H - 1).all() and (boxes[ok, 3] <= W - 1).all()
    assert c.grown == bool((boxes != tight).any())
    assert any(m[:, W - 1].all() for m in masks)                                         # a mask in the last column
    for edge in (256, 512):
        if W > edge:
            assert any(m[:, edge - 1].any() and m[:, edge].any() for m in masks)         # across two x-blocks of 256 threads
    assert counts.max() >= 30 * H                                                        # many adds to one counter
    if seg is not None:
        assert set(seg.tolist()) == {0, 1, 3, 4} and c.n_seg == 6
        assert not counts[2].any() and not counts[5].any()
        for col, n in T.threshold_columns(W):
            assert counts[3, col] == n
        assert sorted(n for _, n in T.threshold_columns(W)) == [5, 6, 25, 26]
        assert len({col for col, _ in T.threshold_columns(W)}) == 4
        assert (counts[3] > 5).sum() == 3 and (counts[3] > 25).sum() == 1


def test_the_count_frames():
    assert {c.frame for c in T.COUNT_CASES} == {(20, 33), (40, 70), (12, 300), (9, 513)}
    assert {(c.use_seg, c.grown) for c in T.COUNT_CASES} == {(a, b) for a in (False, True) for b in (False, True)}


# ------------------------------------------------------------------------------------------------------- packed words
@pytest.mark.parametrize("W", [1, 31, 32, 33, 64, 77, 300])
def test_pack_and_unpack_round_trip(W):
    rng = np.random.default_rng(W)
    dense = rng.random((3, 5, W)) < 0.5
    wpr = (W + 31) // 32
    for pad_ones in (False, True):
        words = REF.pack(dense, W, pad_ones=pad_ones)
        assert words.shape == (3, 5, wpr) and words.dtype == np.uint32
        got, pad = REF.unpack(words, W)
        assert np.array_equal(got, dense) and pad.shape == (3, 5, wpr * 32 - W)
        assert pad.all() if pad_ones else not pad.any()
    # the layout itself: pixel x is bit x & 31 of word x >> 5 (and the package's own host packer agrees)
    one = np.zeros((1, 1, W), dtype=bool)
    one[0, 0, W - 1] = True
    words = REF.pack(one, W)
    assert int(words[0, 0, (W - 1) >> 5]) == 1 << ((W - 1) & 31) and int(words.astype(np.uint64).sum()) == 1 << ((W - 1) & 31)
    import paste_ref
    assert np.array_equal(REF.pack(dense, W), paste_ref.pack_bits(dense))
