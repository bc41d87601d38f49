"""Crop-framed mask sets (``deepemia_amd/cropset.py``, ``csrc/cropops.hip``, ``csrc/maskwords.h``) against their full-frame forms:
every comparison is ``torch.equal`` / byte equality -- the two frames hold the same bits, so nothing here has a tolerance.  Where
both frames run ONE kernel over a word source (pair counts, gray histogram, pooled gather) a dense NumPy answer stands beside them.

Boxes are (y0, x0, y1, x1) everywhere, as in the C ABI."""
import json
import os
import types

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

pytestmark = pytest.mark.gpu

H, W = 96, 200            # W is no multiple of 32: 7 words per row, the last one partly used
TILE = 64
OFFSETS = [(0, 0),        # flush in the frame's corner
           (150, 50),     # clipped by the right and the bottom frame edge
           (136, 32),     # flush with the right and bottom edge: reaches the frame's last column
           (37, 11)]      # word-unaligned


@pytest.fixture(scope="module")
def ops(gpu_device):
    from deepemia_amd.maskset import MaskOps
    return MaskOps(gpu_device)


def _tile_masks(s: int, seed: int) -> np.ndarray:
    """The mask list of the kernel tests in an s x s tile frame that is placed as a 64 x 64 tile; features are put where the
    nearest rule maps given DESTINATION pixels, so they survive the resize."""
    from deepemia_amd.cropset import nearest_index
    ix = nearest_index(TILE, s)
    g = np.random.default_rng(seed)
    m = []
    m.append(np.zeros((s, s), bool))                                           # empty
    for ty, tx in ((5, 32), (6, 31), (20, 63)):                                # bit 0 / bit 31 of a word (offset (0, 0)); last tile column
        a = np.zeros((s, s), bool)
        a[ix[ty], ix[tx]] = True
        m.append(a)
    a = np.zeros((s, s), bool); a[ix[9], ix[3]:ix[60] + 1] = True; m.append(a)                # one row
    a = np.zeros((s, s), bool); a[ix[2]:ix[61] + 1, ix[33]] = True; m.append(a)               # one column
    a = np.zeros((s, s), bool); a[ix[10]:ix[30] + 1, ix[28]:ix[36] + 1] = True; m.append(a)   # straddles a word boundary
    m.append(np.ones((s, s), bool))                                            # fills its tile
    yy, xx = np.mgrid[0:s, 0:s]
    for _ in range(4):                                                         # random blobs
        cy, cx, ry, rx = g.uniform(0, s), g.uniform(0, s), g.uniform(2, s / 3), g.uniform(2, s / 3)
        m.append((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0) & (g.random((s, s)) < 0.9))
    return np.stack(m)


def _blob_planes(ops, n, h, w, seed, max_box=40, dup=True):
    """n random blobs (boxes <= max_box) as planes, with empties, identical masks and boxes that touch without overlapping."""
    g = np.random.default_rng(seed)
    dense = np.zeros((n, h, w), bool)
    yy, xx = np.mgrid[0:h, 0:w]
    for i in range(n):
        bh, bw = g.integers(1, max_box + 1), g.integers(1, max_box + 1)
        y0, x0 = g.integers(0, h - bh + 1), g.integers(0, w - bw + 1)
        cy, cx = y0 + (bh - 1) / 2, x0 + (bw - 1) / 2
        dense[i] = (((yy - cy) / (bh / 2 + 0.3)) ** 2 + ((xx - cx) / (bw / 2 + 0.3)) ** 2 <= 1.0)
        dense[i, :y0] = False; dense[i, y0 + bh:] = False; dense[i, :, :x0] = False; dense[i, :, x0 + bw:] = False
    if dup and n >= 8:
        dense[1] = dense[0]                                                     # identical masks
        dense[n - 1] = dense[n - 2]
        dense[2] = False                                                        # an empty mask
        dense[3] = False; dense[3, 10:20, 10:20] = True                         # boxes that touch ...
        dense[4] = False; dense[4, 10:20, 20:30] = True                         # ... but do not overlap
        dense[5] = False; dense[5, 20:25, 12:32] = True                         # ... and one below, ending at a word boundary
    ops.set_frame_width(w)
    return ops.from_dense(dense).contiguous()


def _loose_set(ops, planes, w, seed):
    """planes -> a CropMaskSet whose ROOMS are the tight boxes grown by 0 .. 37 pixels per side (clipped): rooms wider than the
    boxes, with other strides, as a placement's upper bounds are."""
    from deepemia_amd.cropset import CropMaskSet
    ops.set_frame_width(w)
    area, bbox = ops.area_bbox(planes)
    bb = bbox.cpu().numpy()
    g = np.random.default_rng(seed)
    room = bb.copy()
    grow = g.integers(0, 38, size=bb.shape)
    h = int(planes.shape[1])
    room[:, 0] = np.maximum(bb[:, 0] - grow[:, 0], 0); room[:, 1] = np.maximum(bb[:, 1] - grow[:, 1], 0)
    room[:, 2] = np.minimum(bb[:, 2] + grow[:, 2], h - 1); room[:, 3] = np.minimum(bb[:, 3] + grow[:, 3], w - 1)
    room[bb[:, 0] < 0] = -1
    cs = CropMaskSet.from_planes(ops, planes, w, bbox=room, area=area.cpu().numpy())
    cs.bbox = bbox                                                              # the TIGHT boxes, as the contract has them
    return cs, area, bbox


# ---------------------------------------------------------------------------------------------------------------- place
@pytest.mark.parametrize("s", [128, 64, 96], ids=["2x_undone", "1x", "1.5x"])
@pytest.mark.parametrize("loose", [False, True], ids=["bound", "grown_rooms"])
def test_place_equals_place_tiles_planes(ops, s, loose):
    from deepemia_amd.cropset import CropMaskSet, rooms_of_placed_tiles
    base = _tile_masks(s, 7)
    dense = np.concatenate([base] * len(OFFSETS))
    xo = [o[0] for o in OFFSETS for _ in range(len(base))]
    yo = [o[1] for o in OFFSETS for _ in range(len(base))]
    ops.set_frame_width(s)
    src = ops.from_dense(dense).contiguous()
    _, sbb = ops.area_bbox(src)
    ref = ops.place_tiles(src, xo, yo, TILE, TILE, H, W, src_w=s)
    ops.set_frame_width(W)
    rarea, rbbox = ops.area_bbox(ref)
    rooms = rooms_of_placed_tiles(sbb.cpu().numpy(), (s, s), (TILE, TILE), xo, yo, (H, W))
    rb = rbbox.cpu().numpy()
    inside = (rb[:, 0] < 0) | ((rooms[:, 0] <= rb[:, 0]) & (rooms[:, 1] <= rb[:, 1]) & (rooms[:, 2] >= rb[:, 2]) & (rooms[:, 3] >= rb[:, 3]))
    assert inside.all()                                                         # the host's rooms contain the tight boxes
    if loose:
        ok = rooms[:, 0] >= 0
        rooms[ok, 0] = np.maximum(rooms[ok, 0] - 3, 0); rooms[ok, 1] = np.maximum(rooms[ok, 1] - 33, 0)
        rooms[ok, 2] = np.minimum(rooms[ok, 2] + 2, H - 1); rooms[ok, 3] = np.minimum(rooms[ok, 3] + 40, W - 1)
    cs = CropMaskSet.place_tiles(ops, src, rooms, xo, yo, TILE, TILE, H, W, src_w=s)
    assert int(rarea.max()) > 0 and int((rbbox[:, 3] == W - 1).sum()) > 0       # something reaches the frame's last column
    assert torch.equal(cs.to_planes(), ref)
    assert torch.equal(cs.area, rarea) and torch.equal(cs.bbox, rbbox)
    lens = (rooms[:, 2] - rooms[:, 0] + 1) * ((rooms[:, 3] >> 5) - (rooms[:, 1] >> 5) + 1) * (rooms[:, 0] >= 0)
    assert np.array_equal(cs.offsets_h, np.concatenate(([0], np.cumsum(lens)[:-1])))


def test_place_with_no_masks(ops):
    from deepemia_amd.cropset import CropMaskSet
    src = torch.zeros((0, 128, 4), dtype=torch.int32, device=ops.device)
    cs = CropMaskSet.place_tiles(ops, src, np.zeros((0, 4), np.int32), [], [], TILE, TILE, H, W, src_w=128)
    assert len(cs) == 0 and tuple(cs.to_planes().shape) == (0, H, 7) and tuple(cs.bbox.shape) == (0, 4)


# ---------------------------------------------------------------------------------------------------------- pair counts
SEGS = [1, 2, 65, 130]


@pytest.fixture(scope="module")
def pair_env(ops):
    n = sum(SEGS)
    planes = _blob_planes(ops, n, H, W, 11)
    planes[70] = planes[3 + 64]; planes[71] = planes[3 + 64]                    # identical masks inside the 130-mask segment
    cs, area, bbox = _loose_set(ops, planes, W, 12)
    first = np.repeat(np.concatenate(([0], np.cumsum(SEGS)[:-1])), SEGS).astype(np.int32)
    count = np.repeat(SEGS, SEGS).astype(np.int32)
    return dict(planes=planes, cs=cs, area=area, bbox=bbox, first=first, count=count, n=n, G=_dense_counts(ops, planes, W))


def _dense_counts(ops, planes, w):
    """G[i, j] = |mask_i & mask_j| from the unpacked masks (every count is below 2^24, so the float32 product is exact)."""
    D = ops.to_dense(planes, w).reshape(int(planes.shape[0]), -1).astype(np.float32)
    return (D @ D.T).astype(np.int32)


def _dense_pair_matrix(G, first, count, label, ld):
    """The [n, ld] layout of ``pair_matrix`` from G: |i & j| at [i, j - first[i]] for j > i of i's segment with an equal label."""
    want = np.zeros((len(first), ld), np.int32)
    for i in range(len(first)):
        for j in range(i + 1, int(first[i]) + int(count[i])):
            if j - first[i] < ld and (label is None or label[i] == label[j]):
                want[i, j - first[i]] = G[i, j]
    return want


@pytest.mark.parametrize("labels", ["none", "one_per_segment", "mixed"])
@pytest.mark.parametrize("ld", [130, 64])
def test_pair_matrix_equals_plane_kernel(ops, pair_env, labels, ld):
    e = pair_env
    g = np.random.default_rng(5)
    label = {"none": None, "one_per_segment": np.repeat(np.arange(len(SEGS)), SEGS).astype(np.int32),
             "mixed": g.integers(0, 3, e["n"]).astype(np.int32)}[labels]
    ops.set_frame_width(W)
    ref = ops.pair_matrix(e["planes"], e["bbox"], e["first"], e["count"], label, ld)
    got = e["cs"].pair_matrix(e["first"], e["count"], label, ld)
    assert int((ref > 0).sum()) > 50                                             # the blobs do overlap (mixed labels count a third of the pairs)
    assert torch.equal(got, ref)
    assert np.array_equal(ref.cpu().numpy(), _dense_pair_matrix(e["G"], e["first"], e["count"], label, ld))


def test_pair_intersections_equal_plane_kernel(ops, pair_env):
    e = pair_env
    g = np.random.default_rng(6)
    perm = g.permutation(e["n"])
    other = e["cs"].select(perm)
    planes_b = e["planes"][torch.from_numpy(perm).to(ops.device)].contiguous()
    pi = np.concatenate([g.integers(0, e["n"], 400), np.arange(8), [2, 2, 0, 9]]).astype(np.int64)          # random, (i, i), an empty member
    pj = np.concatenate([g.integers(0, e["n"], 400), np.arange(8), [0, 2, 2, 2]]).astype(np.int64)
    ops.set_frame_width(W)
    ref_aa = ops.pair_intersections(e["planes"], e["planes"], e["bbox"], e["bbox"], pi, pj)
    assert np.array_equal(e["cs"].pair_intersections(e["cs"], pi, pj), ref_aa)
    assert np.array_equal(ref_aa, e["G"][pi, pj])
    assert int(e["area"][2]) == 0 and ref_aa[-3] == 0 and ref_aa[400] == int(e["area"][0]) > 0
    bbox_b = e["bbox"][torch.from_numpy(perm).to(ops.device)].contiguous()
    ref_ab = ops.pair_intersections(e["planes"], planes_b, e["bbox"], bbox_b, pi, pj)
    assert np.array_equal(e["cs"].pair_intersections(other, pi, pj), ref_ab) and int(ref_ab.sum()) > 0
    assert np.array_equal(ref_ab, e["G"][pi, perm[pj]])


def test_long_windows_in_both_frames_against_dense_numpy(ops):
    """The stages that are ONE kernel over a word source, on windows of every length: two nearly-full-frame masks (a shared window
    of 96 x 7 words: ten trips per lane of the matrix kernel's wave and a remainder after any unroll factor), a full-width row,
    a full-height column in the frame's partly used last word, the frame's last pixel and an empty mask -- from planes and
    from a set with grown rooms, against dense NumPy and against each other."""
    from deepemia_amd.maskset import PlanePool
    g = np.random.default_rng(51)
    dense = np.zeros((6, H, W), bool)
    dense[0] = g.random((H, W)) < 0.9; dense[0, [0, -1], :] = True; dense[0, :, [0, -1]] = True
    dense[1] = g.random((H, W)) < 0.8; dense[1, [0, -1], :] = True; dense[1, :, [0, -1]] = True
    dense[2, 40, :] = True
    dense[3, :, 197] = True
    dense[4, H - 1, W - 1] = True
    n = len(dense)
    ops.set_frame_width(W)
    planes = ops.from_dense(dense).contiguous()
    cs, area, bbox = _loose_set(ops, planes, W, 52)
    G = (dense.reshape(n, -1).astype(np.int32) @ dense.reshape(n, -1).T.astype(np.int32)).astype(np.int32)
    assert np.array_equal(bbox.cpu().numpy()[:2], [[0, 0, H - 1, W - 1]] * 2) and G[0, 1] > 10000 and G[2, 3] == 1 and G[1, 4] == 1 and G[5].sum() == 0
    # every pair of one segment, and every listed pair (i, j) in both orders
    first, count = np.zeros(n, np.int32), np.full(n, n, np.int32)
    want = _dense_pair_matrix(G, first, count, None, n)
    assert np.array_equal(ops.pair_matrix(planes, bbox, first, count, None, n).cpu().numpy(), want)
    assert np.array_equal(cs.pair_matrix(first, count, None, n).cpu().numpy(), want)
    pi, pj = [a.ravel().astype(np.int64) for a in np.mgrid[0:n, 0:n]]
    assert np.array_equal(ops.pair_intersections(planes, planes, bbox, bbox, pi, pj), G[pi, pj])
    assert np.array_equal(cs.pair_intersections(cs, pi, pj), G[pi, pj])
    # gray histogram: BGR through OpenCV's fixed point, and a gray image as it is
    bgr = g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    gray = ((bgr[..., 0].astype(np.int64) * 1868 + bgr[..., 1].astype(np.int64) * 9617 + bgr[..., 2].astype(np.int64) * 4899 + (1 << 13)) >> 14)
    for img, lv in ((bgr, gray), (np.ascontiguousarray(bgr[..., 1]), bgr[..., 1])):
        hist = np.stack([np.bincount(lv[d], minlength=256) for d in dense])
        dev = torch.from_numpy(img).to(ops.device)
        assert np.array_equal(ops.gray_histogram(planes, dev, bbox), hist) and np.array_equal(cs.gray_histogram(dev), hist)
    # pooled gather, twice through the same slots: the second pass puts small boxes where large ones were
    pool_p, pool_c = PlanePool(ops.device, H, (W + 31) // 32, n), PlanePool(ops.device, H, (W + 31) // 32, n)
    bb = bbox.cpu().numpy()
    for order in (np.arange(n), np.array([4, 5, 3, 0, 1, 2])):
        it = torch.from_numpy(order).to(ops.device)
        ops.gather_regions_pooled(planes, order, bb[order], pool_p, grow=1)
        cs.select(order).unpack_pooled(pool_c, 0, n, grow=1)
        grown = np.stack([np.maximum(bb[order, 0] - 1, 0), np.maximum(bb[order, 1] - 1, 0),
                          np.minimum(bb[order, 2] + 1, H - 1), np.minimum(bb[order, 3] + 1, W - 1)], axis=1)
        grown[bb[order, 0] < 0] = -1
        for pool in (pool_p, pool_c):
            assert np.array_equal(ops.to_dense(pool.planes, W), dense[order]) and torch.equal(pool.planes, planes[it])
            assert np.array_equal(pool.prev.cpu().numpy(), grown)


# ------------------------------------------------------------------------------------------------ gather / select / cat
def test_select_and_gather_round_trip_through_planes(ops, pair_env):
    e = pair_env
    g = np.random.default_rng(8)
    idx = np.concatenate([g.permutation(e["n"])[:90], [2, 2, 0, 0, 1, 197]])     # permuted, repeated, empty members
    it = torch.from_numpy(idx).to(ops.device)
    sub = e["cs"].select(idx)
    assert torch.equal(sub.to_planes(), e["planes"][it])
    assert torch.equal(sub.bbox, e["bbox"][it]) and torch.equal(sub.area, e["area"][it])
    assert np.array_equal(sub.room_h, e["cs"].room_h[idx]) and torch.equal(sub.room.cpu(), torch.from_numpy(sub.room_h))
    assert len(e["cs"].select([])) == 0
    again = sub.select(np.arange(len(idx))[::-1])
    assert torch.equal(again.to_planes(), e["planes"][it.flip(0)])


def test_cat_round_trip_through_planes(ops, pair_env):
    from deepemia_amd.cropset import CropMaskSet
    e = pair_env
    a, b, c = e["cs"].select(np.arange(0, 40)), e["cs"].select([2, 2]), e["cs"].select(np.arange(150, 198))
    ops.set_frame_width(W)
    d = CropMaskSet.from_planes(ops, e["planes"][40:60].contiguous(), W)          # tight rooms beside grown ones
    allc = CropMaskSet.cat([a, CropMaskSet.empty(ops, (H, W)), b, d, c])
    it = torch.cat([torch.arange(0, 40), torch.tensor([2, 2]), torch.arange(40, 60), torch.arange(150, 198)]).to(ops.device)
    assert torch.equal(allc.to_planes(), e["planes"][it])
    assert torch.equal(allc.bbox, e["bbox"][it]) and torch.equal(allc.area, e["area"][it])
    assert np.array_equal(allc.offsets_h, torch.as_tensor(allc.offsets).cpu().numpy()) and allc.offsets_h[0] == 0
    assert np.all(np.diff(allc.offsets_h) >= 0) and allc.words == int(a.words + b.words + c.words + d.words)


def test_from_planes_with_index_copies_no_plane(ops, pair_env):
    from deepemia_amd.cropset import CropMaskSet
    e = pair_env
    idx = [5, 0, 2, 120, 64]
    cs = CropMaskSet.from_planes(ops, e["planes"], W, bbox=e["bbox"].cpu().numpy(), area=e["area"].cpu().numpy(), index=idx)
    it = torch.tensor(idx, device=ops.device)
    assert torch.equal(cs.to_planes(), e["planes"][it]) and torch.equal(cs.area, e["area"][it]) and torch.equal(cs.bbox, e["bbox"][it])


# -------------------------------------------------------------------------------------------------------- unpack_pooled
def test_unpack_pooled_three_chunks_through_a_pool_of_four(ops):
    from deepemia_amd.maskset import PlanePool
    planes = _blob_planes(ops, 12, H, W, 21, max_box=60)
    order = [0, 6, 2, 7, 1, 8, 3, 9, 4, 10, 5, 11]                              # big and small boxes, an empty one, in turn per slot
    planes = planes[torch.tensor(order, device=ops.device)].contiguous()
    cs, _, bbox = _loose_set(ops, planes, W, 22)
    pool = PlanePool(ops.device, H, (W + 31) // 32, 4)
    scratch = torch.empty_like(pool.planes)
    ops.set_frame_width(W)
    for f in (0, 4, 8):
        view = cs.unpack_pooled(pool, f, 4)
        fresh = cs.to_planes(f, 4)
        assert torch.equal(fresh, planes[f:f + 4])
        assert torch.equal(pool.planes, fresh)                                  # everywhere: outside the boxes as well
        a, b = ops.trace(view, max_contours=64, bbox=bbox[f:f + 4], scratch=scratch), ops.trace(fresh, max_contours=64, bbox=bbox[f:f + 4])
        (ca, ia, ra, ua), (cb, ib, rb, ub) = a.host(), b.host()
        assert ua == ub and np.array_equal(ca, cb) and np.array_equal(ia[..., :3], ib[..., :3]) and np.array_equal(ra, rb)
        for qa, qb in zip(a.records(measure=False), b.records(measure=False)):   # (a contour's place in the point pool is not part of the table)
            assert len(qa) == len(qb) and all(np.array_equal(x["points"], y["points"]) for x, y in zip(qa, qb))
        nb = bbox[f:f + 4]
        assert torch.equal(pool.prev, nb)                                        # grow = 0: the recorded boxes are the new ones
    cs.unpack_pooled(pool, 2, 1)                                                # a short chunk leaves the other slots alone
    assert torch.equal(pool.planes[0], planes[2]) and torch.equal(pool.planes[1:], planes[9:12])


# ------------------------------------------------------------------------------------------------------ decision equality
def _fake_pipe(dev, frame):
    from deepemia_amd.functions.inference import InferencePipeline
    return InferencePipeline([types.SimpleNamespace(engine=types.SimpleNamespace(device=torch.device(dev)))], "t", {"mask_frame": frame}, {})


@pytest.fixture(scope="module")
def detections(gpu_device):
    """>= 200 random overlapping detections over 3 classes on a 256 x 320 frame, class-major (as the image loop appends them)."""
    pf, pc = _fake_pipe(gpu_device, "full"), _fake_pipe(gpu_device, "crop")
    n, h, w = 240, 256, 320
    planes = _blob_planes(pf.ops, n, h, w, 31, max_box=70)
    g = np.random.default_rng(32)
    classes = np.sort(g.integers(0, 3, n)).tolist()
    scores = g.permutation(n).astype(np.float64) / n * 0.7 + 0.3               # all different: a score names its detection
    return dict(pf=pf, pc=pc, planes=planes, classes=classes, scores=scores.tolist(), n=n, h=h, w=w)


@pytest.mark.parametrize("thr, all_pairs", [(0.4, False), (0.7, False), (0.7, True)])
def test_smart_dedup_decisions_equal_full_frame(detections, thr, all_pairs):
    from deepemia_amd.cropset import CropMaskSet
    d = detections
    for p in (d["pf"], d["pc"]):
        p.ops.set_frame_width(d["w"])
    cs = CropMaskSet.from_planes(d["pc"].ops, d["planes"], d["w"])
    mf, sf, cf, tf = d["pf"].deduplicate_masks_smart(d["planes"], d["scores"], d["classes"], thr, with_tables=True, all_pairs=all_pairs)
    mc, sc, cc, tc = d["pc"].deduplicate_masks_smart(cs, d["scores"], d["classes"], thr, with_tables=True, all_pairs=all_pairs)
    assert 20 < len(sf) < d["n"]                                                # the filter removes some and keeps some
    assert sc == sf and cc == cf                                                # exactly the same detections, same order
    assert isinstance(mc, CropMaskSet) and torch.equal(mc.to_planes(), mf)
    assert np.array_equal(tc[0], tf[0]) and np.array_equal(tc[1], tf[1])
    assert (tc[2] is None and tf[2] is None) or np.array_equal(tc[2], tf[2])


def test_merge_segments_and_constraints_equal_full_frame(detections):
    from deepemia_amd.cropset import CropMaskAlgebra, CropMaskSet
    from deepemia_amd.utils.mask_algebra import DeviceMaskAlgebra
    from deepemia_amd.utils.spatial_constraints import apply_spatial_constraints_indices
    d = detections
    cl = np.asarray(d["classes"])
    segs = [(int(np.searchsorted(cl, c, "left")), int(np.searchsorted(cl, c, "right"))) for c in range(3)]
    cs = CropMaskSet.from_planes(d["pc"].ops, d["planes"], d["w"])
    of = d["pf"].deduplicate_masks_smart_segments(d["planes"], d["scores"], d["classes"], segs, 0.4)
    oc = d["pc"].deduplicate_masks_smart_segments(cs, d["scores"], d["classes"], segs, 0.4)
    for (mf, sf, cf, _), (mc, sc, cc, _) in zip(of, oc):
        assert sc == sf and cc == cf and len(sf) > 0 and torch.equal(mc.to_planes(), mf)
    # the spatial constraints over the merged set: the algebra asks the listed-pairs kernel (nothing preloaded)
    parts_f, parts_c = [o[0] for o in of], [o[0] for o in oc]
    scores, classes = [s for o in of for s in o[1]], [c for o in of for c in o[2]]
    pf_, pc_ = torch.cat(parts_f), CropMaskSet.cat(parts_c)
    cfg = {"enabled": True, "containment_threshold": 0.3, "containment_rules": {1: 0},
           "overlap_rules": {0: {"allow_overlap": False, "max_iou_threshold": 0.1}, 2: {"allow_overlap": True, "max_iou_threshold": 0.2}}}
    kf = apply_spatial_constraints_indices(DeviceMaskAlgebra(d["pf"].ops, pf_), scores, classes, cfg)
    kc = apply_spatial_constraints_indices(CropMaskAlgebra(pc_), scores, classes, cfg)
    assert kc == kf and 0 < len(kf) < len(scores)


# ------------------------------------------------------------------------------------------------------------------ memory
def test_crop_merge_peaks_below_a_quarter_of_the_full_frame_merge(gpu_device):
    """400 tile masks (boxes <= 40 x 40) on a 1024^2 frame through placement + the 0.4 merge, both frames in one process.
    full: 400 x 128 KiB of planes per stage; crop: under 1 MiB of words + the 32 planes (4 MiB) of the pool."""
    from deepemia_amd.cropset import CropMaskSet, rooms_of_placed_tiles
    h = w = 1024
    tile, n = 256, 400
    pf, pc = _fake_pipe(gpu_device, "full"), _fake_pipe(gpu_device, "crop")
    src = _blob_planes(pf.ops, n, tile, tile, 41, max_box=40, dup=False)
    pf.ops.set_frame_width(tile)
    _, sbb = pf.ops.area_bbox(src)
    sbb = sbb.cpu().numpy()
    g = np.random.default_rng(42)
    xo, yo = (g.integers(0, 5, n) * 192).tolist(), (g.integers(0, 5, n) * 192).tolist()
    scores, classes = (g.permutation(n) / n).tolist(), [0] * n
    out, peak = {}, {}
    for frame, pipe in (("full", pf), ("crop", pc)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        pipe.ops.set_frame_width(w)
        if frame == "full":
            placed = pipe.ops.place_tiles(src, xo, yo, tile, tile, h, w, src_w=tile)
        else:
            placed = CropMaskSet.place_tiles(pipe.ops, src, rooms_of_placed_tiles(sbb, (tile, tile), (tile, tile), xo, yo, (h, w)), xo, yo,
                                             tile, tile, h, w, src_w=tile)
        m, s, c = pipe.deduplicate_masks_smart(placed, scores, classes, 0.4)
        torch.cuda.synchronize()
        peak[frame] = torch.cuda.max_memory_allocated() - base
        out[frame] = (m.to_planes() if frame == "crop" else m, s)
        del placed, m
    print(f"peak allocation: full {peak['full'] / 2**20:.1f} MiB, crop {peak['crop'] / 2**20:.1f} MiB")
    assert out["crop"][1] == out["full"][1] and torch.equal(out["crop"][0], out["full"][0]) and 0 < len(out["full"][1]) < n
    assert peak["crop"] < peak["full"] / 4


# --------------------------------------------------------------------------------------------------------------------- CLI
DATASET = "synthpores"
CLASSES = ["pore", "throat"]


def _write_tree(root, ds_cfg):
    from deepemia_amd import synth
    cfgdir = root / "cfg"
    (cfgdir / "datasets").mkdir(parents=True)
    split = root / "split_dir"
    base = {"bucket": None,
            "paths": {"split_dir": str(split), "category_json": str(root / "dataset_info.json"), "local_dataset_root": str(root)},
            "inference_settings": {"confidence_mode": "auto", "ensemble_settings": {"enabled": False, "small_classes_only": False},
                                   "spatial_constraints": {"default": {"enabled": False}}},
            "measure_contrast_distribution": True,
            "l4_performance_optimizations": {"enable_parallel_mask_processing": True}}
    (cfgdir / "config.yaml").write_text(yaml.safe_dump(base, sort_keys=False))
    (root / "dataset_info.json").write_text(json.dumps({DATASET: ["imgs", "labels", CLASSES]}))
    mdir = split / DATASET / "rcnn_r50"
    mdir.mkdir(parents=True)
    synth.save_d2_checkpoint(str(mdir / "model_final_r50.pth"), synth.random_d2_state_dict(50, len(CLASSES), seed=0, mask_bias=0.5, mask_gain=6.0))
    inf = root / "DATASET" / "INFERENCE"
    inf.mkdir(parents=True)
    for i, (hh, ww) in enumerate(((300, 417), (260, 500))):
        Image.fromarray(np.ascontiguousarray(synth.em_tile(40 + i, 512)[:hh, :ww, ::-1])).save(inf / f"em_{i}.tif")
    return cfgdir, split


def _set_frame(cfgdir, ds_cfg, frame):
    cfg = json.loads(json.dumps(ds_cfg))
    if frame is not None:
        cfg["inference_overrides"]["mask_frame"] = frame
    (cfgdir / "datasets" / f"{DATASET}.yaml").write_text(yaml.safe_dump(cfg, sort_keys=False))


@pytest.mark.parametrize("upscale", [1.0, 2.0])
def test_cli_writes_the_same_bytes_in_both_mask_frames(tmp_path, monkeypatch, gpu_device, upscale):
    import main as cli
    from deepemia_amd.functions import inference as inf_mod
    from deepemia_amd.utils import config as C

    ds_cfg = {"inference_overrides": {"confidence_mode": "manual",
                                      "class_specific_settings": {"class_0": {"confidence_threshold": 0.3, "iou_threshold": 0.6},
                                                                  "class_1": {"confidence_threshold": 0.35, "iou_threshold": 0.5}},
                                      "tile_settings": {"tile_size": 200, "overlap_ratio": 0.125, "upscale_factor": upscale, "edge_filter_enabled": True},
                                      "spatial_constraints": {"enabled": True, "containment_rules": {1: 0}, "containment_threshold": 0.5}}}
    cfgdir, split = _write_tree(tmp_path, ds_cfg)
    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(cfgdir))
    monkeypatch.setenv("DEEPEMIA_OFFLINE", "1")
    monkeypatch.setenv("DEEPEMIA_WORKERS", "1")
    monkeypatch.chdir(tmp_path)
    names = ["measurements_results.csv", "R50_flip_results.csv", "class_color_legend.txt", "em_0.tif_predictions.png", "em_1.tif_predictions.png"]
    outs, stats = {}, {}
    for frame in ("full", "crop"):
        _set_frame(cfgdir, ds_cfg, frame)
        C.reset_cache()
        assert cli.main(["--task", "inference", "--dataset_name", DATASET, "--threshold", "0.3", "--no-gpu-check", "--visualize"]) == 0
        C.reset_cache()
        outs[frame] = {nm: (split / nm).read_bytes() for nm in names}
        stats[frame] = dict(inf_mod.LAST_RUN_STATS)
        for nm in names:
            (split / nm).unlink()
    assert len(outs["full"]["measurements_results.csv"].splitlines()) > 10 and len(outs["full"]["R50_flip_results.csv"].splitlines()) > 10
    for nm in names:
        assert outs["crop"][nm] == outs["full"][nm], nm
    assert stats["full"]["mask_frame"] == "full" and stats["crop"]["mask_frame"] == "crop"
    assert 0 < stats["crop"]["full_frame_planes_peak"] <= stats["crop"]["plane_pool_capacity"] == 32
    assert stats["full"]["full_frame_planes_peak"] > 0
