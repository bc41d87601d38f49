"""GPU tests of the evaluate task's crop scoring (``evaluation.score_frame: crops``): the polygon rasteriser into rooms, the
cross matrix and the run-length encoder over crop-framed sets -- each bit-identical to its plane entry and to the CPU
restatements, with canaries around everything they write -- the peak memory of one image's crop scoring, one small image
through the scorer's three entries (predictor mode, pipeline mode on planes and on crops: the same rows), and
``evaluate_model`` end to end under ``crop_direct`` / ``crops`` against ``full`` / ``planes``."""
import gc
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parent))
import coco_ref as R  # noqa: E402
import coco_ref_ext as X  # noqa: E402
from test_gpu_evaluate_pipeline import CLASSES, DATASET, _configure, _labels, _metrics, _same, _sha  # noqa: E402

pytestmark = pytest.mark.gpu

FRAMES = [(96, 200), (40, 64)]          # W no multiple of 32 (seven word columns); W an exact multiple
CANARY = -1                             # all ones


@pytest.fixture(scope="module")
def ops():
    from deepemia_amd.maskset import MaskOps
    return MaskOps("cuda:0")


def _dev(ops, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)


def _spaced(room_h, gap=3):
    """Offsets that leave ``gap`` canary words before every room and after the last: (offsets [M] i64, total words)."""
    from deepemia_amd.cropset import room_lengths

    lens = room_lengths(room_h)
    off = np.cumsum(lens + gap) - lens
    return off.astype(np.int64), int(off[-1] + lens[-1] + gap) if len(lens) else gap


def _outside(off, lens, total):
    keep = np.ones(total, dtype=bool)
    for o, n in zip(off.tolist(), lens.tolist()):
        keep[o:o + n] = False
    return keep


# ---- the rasteriser -------------------------------------------------------------------------------------------------------------
def _masks(rng, H, W):
    """About 60 masks: concave rings, the label files' 65-point ellipse rings, masks of two polygons, polygons on each edge and in
    each corner, polygons crossing the frame edge, one wholly outside, a sub-pixel sliver, one covering the whole frame."""
    from deepemia_amd.data.datasets import ellipse_polygon

    masks = []
    for i in range(40):
        cx, cy = rng.uniform(8, W - 8), rng.uniform(8, H - 8)
        if i % 3 == 0:
            k = rng.randint(4, 10)
            ang = np.sort(rng.uniform(0, 2 * np.pi, k))
            r = rng.uniform(2, 22, k)
            masks.append([list(np.round(np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1).reshape(-1), 2))])
        elif i % 3 == 1:
            px, py = ellipse_polygon(cx, cy, rng.uniform(2, 18), rng.uniform(2, 18), rng.uniform(0, 180))
            masks.append([[c for x, y in zip(px, py) for c in (x + .5, y + .5)]])
        else:
            x0, y0 = int(cx) - 10, int(cy) - 12
            masks.append([[x0 + .5, y0 + .5, x0 + 18.5, y0 + .5, x0 + 18.5, y0 + 9.5, x0 + .5, y0 + 9.5],
                          [x0 + 12.5, y0 + 4.5, x0 + 30.5, y0 + 6.5, x0 + 14.5, y0 + 22.5]])

    def box(x0, y0, x1, y1):
        return [[x0, y0, x1, y0, x1, y1, x0, y1]]
    # on each edge and in each corner (inside the frame), then across each edge and corner
    for x0, y0 in [(0, H / 2), (W - 9, H / 2), (W / 2, 0), (W / 2, H - 7), (0, 0), (W - 9, 0), (0, H - 7), (W - 9, H - 7)]:
        masks.append(box(x0, y0, x0 + 9, y0 + 7))
    for cx, cy in [(-3, H / 2), (W + 2, H / 2), (W / 2, -4), (W / 2, H + 3), (-2, -2), (W + 1, -3), (-3, H + 2), (W + 2, H + 1)]:
        k = 7
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        r = rng.uniform(6, 16, k)
        masks.append([list(np.round(np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1).reshape(-1), 3))])
    masks.append(box(-40, -30, -20, -10))                                           # wholly outside: empty room
    masks.append([[10.1, 10.1, 10.3, 10.1, 10.2, 10.3]])                            # a sub-pixel sliver: no pixel
    masks.append(box(-1, -1, W + 1, H + 1))                                         # the whole frame: more than one block's work
    return masks


def _crop_rasterize_raw(ops, masks, H, W, room_h, off_h, total):
    """``demia_crop_poly_rasterize`` into a payload of canaries with the caller's offsets: (payload, area, bbox, error word) on the host."""
    from deepemia_amd import _lib
    from deepemia_amd import cocoeval as CE
    from deepemia_amd.cropset import room_lengths

    M = len(masks)
    payload = torch.full((total,), CANARY, dtype=torch.int32, device=ops.device)
    area = torch.full((M + 1,), CANARY, dtype=torch.int32, device=ops.device)
    bbox = torch.full((M + 1, 4), CANARY, dtype=torch.int32, device=ops.device)
    tabs = CE._PolygonTables(ops, masks)
    room_d, off_d = _dev(ops, np.asarray(room_h, dtype=np.int32)), _dev(ops, np.asarray(off_h, dtype=np.int64))      # (alive until the results are fetched)
    _lib.check(ops.lib.demia_crop_poly_rasterize(*tabs.args(), M, H, W, _lib.ptr(room_d), _lib.ptr(off_d), int(room_lengths(room_h).max()),
                                                 _lib.ptr(payload), _lib.ptr(area), _lib.ptr(bbox), ops._stream()), "demia_crop_poly_rasterize")
    area, bbox = area.cpu().numpy(), bbox.cpu().numpy()
    assert area[M] == CANARY and (bbox[M] == CANARY).all()
    return payload.cpu().numpy(), area[:M], bbox[:M], int(tabs.err.cpu().numpy()[0])


@pytest.mark.parametrize("H,W", FRAMES)
def test_rasteriser_into_rooms_equals_the_plane_rasteriser_and_fr_poly(ops, H, W):
    from deepemia_amd import _lib
    from deepemia_amd import cocoeval as CE
    from deepemia_amd.cropset import CropMaskSet, room_lengths

    rng = np.random.RandomState(H + W)
    masks = _masks(rng, H, W)
    M = len(masks)
    planes, p_area, p_bbox = CE.rasterize_polygons(ops, masks, H, W)
    cset, err = CE.rasterize_polygons_crop(ops, masks, H, W)
    CE.check_rasterize_error(int(err.item()))
    room_h = CE.polygon_rooms(masks, H, W)
    assert np.array_equal(cset.room_h, room_h) and len(cset) == M
    lens = room_lengths(room_h)
    assert lens[-1] == H * ((W + 31) // 32) and lens[-3] == 0                               # whole frame; wholly outside
    if (H, W) == FRAMES[0]:
        assert lens[-1] == 672 > 256                                                        # more than one block's work
    # the plane rasteriser's planes cropped to the rooms
    want = torch.full((cset.words + 1,), CANARY, dtype=torch.int32, device=ops.device)
    _lib.check(ops.lib.demia_mask_crop_pack(_lib.ptr(planes), _lib.ptr(cset.room), _lib.ptr(cset.offsets), M, H, W, _lib.ptr(want), ops._stream()),
               "demia_mask_crop_pack")
    assert torch.equal(cset.payload[:cset.words], want[:cset.words])
    assert torch.equal(cset.area, p_area) and torch.equal(cset.bbox, p_bbox)
    # coco_ref's rleFrPoly, pixel by pixel
    crops, area_h, bbox_h = cset.host_crops(), cset.area.cpu().numpy(), cset.bbox.cpu().numpy()
    for m, polys in enumerate(masks):
        ref = R.poly_mask(polys, H, W)
        got = np.zeros((H, W), dtype=bool)
        if crops[m] is not None:
            y0, x0, sub = crops[m]
            got[y0:y0 + sub.shape[0], x0:x0 + sub.shape[1]] = sub
        assert (got == ref).all(), m
        assert area_h[m] == ref.sum()
        ys, xs = np.nonzero(ref)
        assert bbox_h[m].tolist() == ([ys.min(), xs.min(), ys.max(), xs.max()] if len(ys) else [-1] * 4)
    assert area_h[-1] == H * W and area_h[-2] == 0 and area_h[-3] == 0                      # whole frame, sliver, outside
    assert np.count_nonzero(area_h) >= 50 and (area_h[40:48] > 0).all() and np.count_nonzero(area_h[48:56]) >= 4
    # canaries: a guard before every room and behind the last, all ones between calls; exactly the rooms are written
    off_h, total = _spaced(room_h)
    pay, area, bbox, word = _crop_rasterize_raw(ops, masks, H, W, room_h, off_h, total)
    assert word == 0
    assert (pay[_outside(off_h, lens, total)] == CANARY).all()
    ref_pay = cset.payload[:cset.words].cpu().numpy()
    for m in range(M):
        assert np.array_equal(pay[off_h[m]:off_h[m] + lens[m]], ref_pay[cset.offsets_h[m]:cset.offsets_h[m] + lens[m]]), m
    assert np.array_equal(area, area_h) and np.array_equal(bbox, bbox_h)


@pytest.mark.parametrize("H,W", FRAMES)
def test_rooms_that_are_too_small_give_the_error_word_and_no_write_outside_them(ops, H, W):
    from deepemia_amd import _lib
    from deepemia_amd import cocoeval as CE
    from deepemia_amd.cropset import room_lengths

    rng = np.random.RandomState(7)
    masks = _masks(rng, H, W)
    good = CE.polygon_rooms(masks, H, W)
    big = [m for m in range(len(masks)) if good[m, 0] >= 0 and good[m, 2] - good[m, 0] >= 8 and good[m, 3] - good[m, 1] >= 8]
    cuts = {"top": (0, +4), "left": (1, +4), "bottom": (2, -4), "right": (3, -4)}
    for k, (name, (col, d)) in enumerate(cuts.items()):
        small = good.copy()
        m = big[k]
        small[m, col] += d                                      # a room that misses four rows / columns of its mask
        off_h, total = _spaced(small)
        pay, _, _, word = _crop_rasterize_raw(ops, masks, H, W, small, off_h, total)
        assert word == 2, name
        assert (pay[_outside(off_h, room_lengths(small), total)] == CANARY).all(), name
        _, err = CE.rasterize_polygons_crop(ops, masks, H, W, rooms=small)
        with pytest.raises(_lib.HipKernelError, match="outside its mask's room"):
            CE.check_rasterize_error(int(err.item()))
    # a mask with pixels and an EMPTY room
    small = good.copy()
    small[big[0]] = -1
    off_h, total = _spaced(small)
    pay, area, bbox, word = _crop_rasterize_raw(ops, masks, H, W, small, off_h, total)
    assert word == 2 and area[big[0]] == 0 and bbox[big[0]].tolist() == [-1] * 4
    assert (pay[_outside(off_h, room_lengths(small), total)] == CANARY).all()


# ---- the cross matrix -----------------------------------------------------------------------------------------------------------
def _blob_masks(rng, n, H, W, fixed=()):
    """Dense [n, H, W] noisy rectangles; ``fixed`` = (index, y0, x0, y1, x1) boxes drawn solid; every seventh mask empty."""
    dense = np.zeros((n, H, W), dtype=bool)
    for i in range(n):
        if i % 7 == 6:
            continue
        h, w = rng.randint(1, min(H, 40) + 1), rng.randint(1, min(W, 70) + 1)
        y0, x0 = rng.randint(0, H - h + 1), rng.randint(0, W - w + 1)
        dense[i, y0:y0 + h, x0:x0 + w] = rng.rand(h, w) < .8
    for i, y0, x0, y1, x1 in fixed:
        dense[i] = False
        dense[i, y0:y1 + 1, x0:x1 + 1] = True
    return dense


def _pixels(dense):
    n, H, W = dense.shape
    mi, pos = np.nonzero(dense.transpose(0, 2, 1).reshape(n, -1))
    return mi.astype(np.int64), pos.astype(np.int64)


def _grown(rng, bbox_h, H, W, grow=9):
    """Rooms around the tight boxes, grown by up to ``grow`` pixels on every side (clipped): room != tight box, rooms overlap."""
    room = bbox_h.copy()
    ok = room[:, 0] >= 0
    g = rng.randint(0, grow + 1, room.shape)
    room[:, 0] = np.maximum(0, room[:, 0] - g[:, 0])
    room[:, 1] = np.maximum(0, room[:, 1] - g[:, 1])
    room[:, 2] = np.minimum(H - 1, room[:, 2] + g[:, 2])
    room[:, 3] = np.minimum(W - 1, room[:, 3] + g[:, 3])
    room[~ok] = -1
    return room


def _crop_set(ops, rng, dense, W):
    from deepemia_amd.cropset import CropMaskSet

    planes = ops.from_dense(dense)
    ops.set_frame_width(W)
    area, bbox = ops.area_bbox(planes)
    tight = CropMaskSet.from_planes(ops, planes, W)
    cset = tight.reroom(_grown(rng, bbox.cpu().numpy(), dense.shape[1], W))
    assert not np.array_equal(cset.room_h, tight.room_h)
    return planes, area, bbox, cset


@pytest.mark.parametrize("H,W", FRAMES)
def test_cross_matrix_over_rooms_equals_the_plane_entry_and_the_pixel_count(ops, H, W):
    from deepemia_amd import cocoeval as CE

    rng = np.random.RandomState(3 * H + W)
    D, G = 23, 19
    d_dense = _blob_masks(rng, D, H, W, fixed=[(0, 5, 32, 30, 50), (1, 2, 3, 33, 31)])       # a box that starts at x = 32, one that ends at x = 31
    g_dense = _blob_masks(rng, G, H, W, fixed=[(0, 0, 20, H - 1, 45), (1, 10, 32, 20, 63)])
    d_planes, _, d_bbox, d_set = _crop_set(ops, rng, d_dense, W)
    g_planes, _, g_bbox, g_set = _crop_set(ops, rng, g_dense, W)
    assert d_bbox.cpu().numpy()[:2].tolist() == [[5, 32, 30, 50], [2, 3, 33, 31]]
    want = X.cross_counts(_pixels(d_dense), _pixels(g_dense), D, G)
    assert np.count_nonzero(want) > D and (want[6] == 0).all() and (want[:, 6] == 0).all()                # empty masks on both sides
    dl, gl = rng.randint(0, 3, D), rng.randint(0, 3, G)
    for labels in ((dl, gl), (None, None)):
        got = CE.cross_matrix_crop(ops, d_set, labels[0], g_set, labels[1]).cpu().numpy()
        plane = CE.cross_matrix(ops, d_planes, d_bbox, labels[0], g_planes, g_bbox, labels[1], W).cpu().numpy()
        ref = want if labels[0] is None else want * (dl[:, None] == gl[None, :])
        assert got.shape == (D, G) and np.array_equal(got, plane) and np.array_equal(got, ref)
    assert CE.cross_matrix_crop(ops, d_set, dl, g_set.select([]), gl[:0]).shape == (D, 0)


# ---- run lengths ----------------------------------------------------------------------------------------------------------------
def _rle_case(ops, rng, H, W):
    """Dense masks and the set that stores them: noisy blobs; full columns down to the last row; a mask whose tight box starts at
    row 0 in a room that ends above row H - 1 with an all-ones neighbour stored right behind it; single pixels at (0, 0) and at
    (H - 1, W - 1); an empty mask."""
    from deepemia_amd.cropset import CropMaskSet

    n = 14
    dense = _blob_masks(rng, n, H, W)
    dense[2] = False
    dense[2, H - 20:, 10:17] = True                                  # full columns at the bottom edge
    dense[3] = False
    dense[3, :, 33:36] = True                                        # full columns top to bottom: runs go on into the next column
    dense[4] = False
    dense[4, 0:9, 8:20] = rng.rand(9, 12) < .7
    dense[4, 0, 8:20] = True                                         # tight box starts at row 0, every column set there
    dense[5] = False
    dense[5, :, 0:64] = True                                         # the neighbour: 2 H words of all ones (row H - 1 of mask 4's word
                                                                     # column, addressed from mask 4's first word, lies among them)
    dense[7] = False
    dense[7, 0, 0] = True
    dense[8] = False
    dense[8, H - 1, W - 1] = True
    dense[6] = False                                                 # (empty)
    planes = ops.from_dense(dense)
    ops.set_frame_width(W)
    _, bbox = ops.area_bbox(planes)
    bbox_h = bbox.cpu().numpy()
    room = _grown(rng, bbox_h, H, W)
    room[4] = [0, 8, 12, 19]                                         # ends above row H - 1; one word column
    room[5] = [0, 0, H - 1, 63]
    cset = CropMaskSet.from_planes(ops, planes, W).reroom(room)
    pay = cset.payload[:cset.words].cpu().numpy()
    o5 = int(cset.offsets_h[5])
    assert o5 == cset.offsets_h[4] + 13 and (pay[o5:o5 + 2 * H] == -1).all() and H - 1 < 13 + 2 * H      # all ones right behind mask 4's words
    return dense, planes, bbox, cset


@pytest.mark.parametrize("H,W", FRAMES)
def test_run_lengths_over_rooms_equal_the_plane_entry_and_the_cpu_encoding(ops, H, W):
    from deepemia_amd import _lib
    from deepemia_amd import cocoeval as CE

    rng = np.random.RandomState(H * W)
    dense, planes, bbox, cset = _rle_case(ops, rng, H, W)
    n = len(cset)
    want_counts, want_off = CE.rle_counts(ops, planes, bbox, W)
    counts, off = CE.rle_counts_crop(ops, cset)                      # with a wait in between
    assert np.array_equal(off, want_off) and np.array_equal(counts, want_counts)
    mi, pos = _pixels(dense)
    split = np.searchsorted(mi, np.arange(n + 1))
    for i in range(n):
        assert counts[off[i]:off[i + 1]].tolist() == X.encode_pixels(pos[split[i]:split[i + 1]], H * W), i
    assert counts[off[7]:off[8]].tolist() == [0, 1, H * W - 1] and counts[off[8]:off[9]].tolist() == [H * W - 1, 1]
    assert counts[off[6]:off[7]].tolist() == [H * W]
    # enqueued into a sized room, with the caller's own copy of the boxes
    total = int(off[-1])
    n_t, c_t = CE.rle_counts_launch_crop(ops, cset, total + 5, bbox=bbox.clone())
    runs = CE.rle_counts_finish(n_t.cpu().numpy(), c_t.cpu().numpy())
    assert runs is not None and np.array_equal(runs[0], counts) and np.array_equal(runs[1], off)
    tight = CE.rle_counts_finish(*[t.cpu().numpy() for t in CE.rle_counts_launch_crop(ops, cset, total - 1)])
    assert tight is None                                             # one count short: reported as "did not fit"
    # ... and nothing is written past the room: the write pass into a room that ends one count into the last blob's slot, with
    # canaries behind it
    last = int(off[n - 2])
    assert off[n - 1] - last > 1                                     # (mask n - 2 is a blob with several runs, mask n - 1 is empty)
    n_t = torch.empty((n,), dtype=torch.int32, device=ops.device)
    buf = torch.full((last + 1 + 16,), CANARY, dtype=torch.int32, device=ops.device)

    def run(n_ptr, off_t):
        _lib.check(ops.lib.demia_crop_rle_colmajor(_lib.ptr(cset.payload), _lib.ptr(cset.room), _lib.ptr(cset.offsets), _lib.ptr(cset.bbox), n_ptr,
                                                   _lib.ptr(off_t), _lib.ptr(buf) if off_t is not None else 0, n, H, W, ops._stream()),
                   "demia_crop_rle_colmajor")
    run(_lib.ptr(n_t), None)
    assert np.array_equal(n_t.cpu().numpy(), np.diff(off))
    cut = torch.from_numpy(np.minimum(off, last + 1)).to(ops.device)
    run(0, cut)
    got = buf.cpu().numpy()
    assert np.array_equal(got[:last].view(np.uint32), counts[:last]) and (got[last:] == CANARY).all()      # the slots that do not fit are left alone


# ---- one image through both scorers: rows and memory ---------------------------------------------------------------------------------
def _scoring_inputs(ops, size=1024, n=300):
    """A record with ``n`` polygon annotations (boxes <= 60 px) and three run-length crowd regions, and ``n`` detections near them."""
    rng = np.random.RandomState(21)
    anns, centres = [], []
    for i in range(n):
        cx, cy = rng.uniform(35, size - 35, 2)
        k = rng.randint(4, 10)
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        r = rng.uniform(4, 29, k)
        pts = np.round(np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1).reshape(-1), 2)
        anns.append({"segmentation": [[float(v) for v in pts]], "category_id": int(i % 2), "iscrowd": 0, "area": float(rng.uniform(50, 2000)),
                     "bbox": [float(cx - 29), float(cy - 29), float(cx + 29), float(cy + 29)], "bbox_mode": "XYXY_ABS"})
        centres.append((cx, cy))
    for j in range(3):                                               # crowd regions given as run lengths, between the polygons
        m = np.zeros((size, size), dtype=bool)
        y0, x0 = rng.randint(0, size - 50, 2)
        m[y0:y0 + 50, x0:x0 + 40] = rng.rand(50, 40) < .6
        anns.insert(40 * (j + 1), {"segmentation": {"size": [size, size], "counts": X.encode(m)}, "category_id": j % 2, "iscrowd": 1,
                                   "area": float(m.sum()), "bbox": [float(x0), float(y0), float(x0 + 40), float(y0 + 50)], "bbox_mode": "XYXY_ABS"})
    rec = {"file_name": "synthetic.png", "image_id": 0, "height": size, "width": size, "annotations": anns}
    wpr = size // 32
    words = np.zeros((n, size, wpr), dtype=np.uint32)
    for i, (cx, cy) in enumerate(centres):
        h, w = rng.randint(8, 60), rng.randint(8, 60)
        y0 = int(np.clip(cy - h // 2 + rng.randint(-6, 7), 0, size - h))
        x0 = int(np.clip(cx - w // 2 + rng.randint(-6, 7), 0, size - w))
        sub = np.zeros((h, wpr * 32), dtype=bool)
        sub[:, x0:x0 + w] = rng.rand(h, w) < .85
        words[i, y0:y0 + h] = np.packbits(sub.reshape(h, wpr, 32), axis=-1, bitorder="little").view(np.uint32).reshape(h, wpr)
    planes = torch.from_numpy(words.view(np.int32)).to(ops.device)
    ops.set_frame_width(size)
    area, bbox = ops.area_bbox(planes)
    tabs = (area.cpu().numpy(), bbox.cpu().numpy())
    scores = [float(v) for v in rng.uniform(.3, 1, n)]
    classes = [int(v) for v in rng.randint(0, 2, n)]
    return rec, planes, tabs, scores, classes


def test_crop_scoring_peaks_below_a_quarter_of_the_planes_and_gives_the_same_rows(ops):
    from deepemia_amd import cocoeval as CE
    from deepemia_amd.cropset import CropMaskSet
    from deepemia_amd.functions.evaluate_model import _score_pipeline_image

    size, n = 1024, 300
    rec, planes, tabs, scores, classes = _scoring_inputs(ops, size, n)
    ids = {0: 0, 1: 1}
    t_planes = {"bbox": CE.EvalTables(), "segm": CE.EvalTables()}
    rows_planes = _score_pipeline_image(ops, rec, (size, size), planes, scores, classes, tabs, t_planes, ids)
    cset = CropMaskSet.from_planes(ops, planes, size, bbox=tabs[1], area=tabs[0])
    g_planes, g_area, g_bbox = CE.rasterize_polygons(ops, [a["segmentation"] for a in rec["annotations"] if isinstance(a["segmentation"], list)], size, size)
    inter_planes = CE.cross_matrix(ops, planes, cset.bbox, None, g_planes, g_bbox, None, size).cpu().numpy()
    g_area = g_area.cpu().numpy()
    del planes, g_planes
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    t_crops = {"bbox": CE.EvalTables(), "segm": CE.EvalTables()}
    rows_crops = _score_pipeline_image(ops, rec, (size, size), cset, scores, classes, tabs, t_crops, ids)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    plane_bytes = (n + n) * size * (size // 32) * 4                  # what the planes scorer holds for the polygons and the detections
    print(f"crop scoring of {n} x {n + 3} masks at {size}^2: peak {peak / 2**20:.2f} MiB ({(peak - before) / 2**20:.2f} MiB above the set), "
          f"planes {plane_bytes / 2**20:.1f} MiB")
    assert peak < plane_bytes / 4
    # the same rows: result entries (strings, boxes, scores), pixel counts, IoU tables
    assert rows_crops == rows_planes and len(rows_crops["instances"]) == n
    for task in ("bbox", "segm"):
        for name in ("d_img", "d_cat", "d_score", "d_area", "d_row", "g_img", "g_cat", "g_area", "g_crowd", "g_col", "iou"):
            assert np.array_equal(t_crops[task].cat(name), t_planes[task].cat(name)), (task, name)
    assert np.count_nonzero(t_crops["segm"].cat("iou")) > n // 2
    # ... and the intersections and ground-truth pixel counts themselves, polygons only
    poly = [a for a in rec["annotations"] if isinstance(a["segmentation"], list)]
    gt, err = CE.rasterize_polygons_crop(ops, [a["segmentation"] for a in poly], size, size)
    inter = CE.cross_matrix_crop(ops, cset, None, gt, None).cpu().numpy()
    CE.check_rasterize_error(int(err.item()))
    assert np.array_equal(inter, inter_planes) and np.array_equal(gt.area.cpu().numpy(), g_area)


class _FakeInstances:
    """What the predictor mode's entry reads of an ``Instances``."""

    def __init__(self, image_size, packed_masks, pred_classes, pred_boxes, scores):
        self.image_size, self.packed_masks, self.pred_classes, self.pred_boxes, self.scores = image_size, packed_masks, pred_classes, pred_boxes, scores

    def __len__(self):
        return len(self.scores)


def test_the_three_entries_of_the_scorer_give_the_same_rows_for_the_same_masks(ops):
    """Five detections (one empty) against four annotations (one given as run lengths, one a crowd region, one of another class) at
    70 x 100 (four words per row, the last one partial), boundary AP at width 2 and the outline report on: the predictor mode's
    entry, the pipeline entry on planes and the pipeline entry on a ``CropMaskSet`` give the same ``segm`` and ``boundary`` IoU
    tables, the same run-length strings and the same outline rows; ``bbox`` is the same on planes and crops, and for the predictor
    entry it is ``box_iou`` of the boxes it was given."""
    from deepemia_amd import cocoeval as CE
    from deepemia_amd.cropset import CropMaskSet
    from deepemia_amd.functions.evaluate_model import _gt_box_xywh, _new_tables, _score_image, _score_pipeline_image

    H, W = 70, 100
    rng = np.random.RandomState(4)
    dense = np.zeros((5, H, W), dtype=bool)
    dense[0, 5:30, 20:60] = True                                      # (across the first word boundary)
    dense[1, 35:65, 60:100] = True                                    # (up to the last column, in the partial word)
    dense[3, 40:60, 5:40] = rng.rand(20, 35) < .8                     # dense[2] stays empty
    dense[4, 2:12, 70:95] = True
    runs = np.zeros((H, W), dtype=bool)
    runs[36:66, 58:98] = True

    def poly(x0, y0, x1, y1):
        return [[x0, y0, x1, y0, x1, y1, x0, y1]]
    anns = [{"segmentation": poly(19.5, 4.5, 61.5, 31.5), "category_id": 0, "iscrowd": 0, "area": 1100.0, "bbox": [19.5, 4.5, 61.5, 31.5], "bbox_mode": "XYXY_ABS"},
            {"segmentation": {"size": [H, W], "counts": X.encode(runs)}, "category_id": 1, "iscrowd": 0, "area": 1200.0, "bbox": [58.0, 36.0, 40.0, 30.0],
             "bbox_mode": "XYWH_ABS"},
            {"segmentation": poly(0.0, 38.0, 50.0, 68.0), "category_id": 0, "iscrowd": 1, "area": 1500.0, "bbox": [0.0, 38.0, 50.0, 30.0], "bbox_mode": "XYWH_ABS"},
            {"segmentation": poly(69.5, 1.5, 95.5, 12.5), "category_id": 0, "iscrowd": 0, "area": 280.0, "bbox": [69.5, 1.5, 26.0, 11.0], "bbox_mode": "XYWH_ABS"}]
    rec = {"file_name": "synthetic.png", "image_id": 0, "height": H, "width": W, "annotations": anns}
    classes, scores = [0, 1, 0, 0, 1], [0.875, 0.75, 0.625, 0.5, 0.375]                       # (exact in float32)
    boxes = np.asarray([[19.0, 4.0, 61.5, 31.0], [58.5, 34.0, 100.0, 66.0], [1.0, 2.0, 3.0, 4.5], [4.0, 39.0, 41.0, 61.0], [69.0, 1.0, 96.0, 13.0]], np.float32)
    planes = ops.from_dense(dense)
    ops.set_frame_width(W)
    area, bbox = ops.area_bbox(planes)
    tabs = (area.cpu().numpy(), bbox.cpu().numpy())
    assert planes.shape == (5, H, 4) and tabs[0][2] == 0
    ids, boundary = {0: 0, 1: 1}, (CE.BOUNDARY_RATIO, 2)
    inst = _FakeInstances((H, W), planes, torch.tensor(classes, device=ops.device), torch.from_numpy(boxes).to(ops.device),
                          torch.tensor(scores, dtype=torch.float32, device=ops.device))
    got = {}
    for entry in ("predictor", "planes", "crops"):
        tables, report = _new_tables(boundary), CE.OutlineReport(0.5, 2)
        if entry == "predictor":
            rows = _score_image(ops, rec, inst, tables, ids, boundary, report)
        else:
            masks = planes if entry == "planes" else CropMaskSet.from_planes(ops, planes, W, bbox=tabs[1], area=tabs[0])
            rows = _score_pipeline_image(ops, rec, (H, W), masks, scores, classes, tabs, tables, ids, entry, boundary, report)
        got[entry] = (rows["instances"], tables, report)
    want = got["planes"]
    assert len(want[0]) == 5 and len(want[2].rows) >= 2 and list(want[1]) == ["bbox", "segm", "boundary"]
    assert np.count_nonzero(want[1]["segm"].cat("iou")) >= 3 and (want[1]["boundary"].cat("iou") < want[1]["segm"].cat("iou")).any()
    assert CE.rle_from_string(want[0][2]["segmentation"]["counts"]).tolist() == [H * W]      # the empty detection
    for entry in ("predictor", "crops"):
        inst_rows, tables, report = got[entry]
        for task in ("segm", "boundary"):
            assert np.array_equal(tables[task].cat("iou"), want[1][task].cat("iou")), (entry, task)
        assert [r["segmentation"] for r in inst_rows] == [r["segmentation"] for r in want[0]], entry
        assert [(r["category_id"], r["score"]) for r in inst_rows] == [(r["category_id"], r["score"]) for r in want[0]], entry
        assert report.rows == want[2].rows and report.counts == want[2].counts, entry
    assert got["crops"][0] == want[0] and np.array_equal(got["crops"][1]["bbox"].cat("iou"), want[1]["bbox"].cat("iou"))
    xywh = boxes.copy()
    xywh[:, 2:] -= xywh[:, :2]
    assert [r["bbox"] for r in got["predictor"][0]] == xywh.tolist()
    g_box = np.asarray([_gt_box_xywh(a) for a in anns], dtype=np.float64)
    crowd = np.asarray([a["iscrowd"] for a in anns], dtype=np.uint8)
    assert np.array_equal(got["predictor"][1]["bbox"].cat("iou"), CE.box_iou(xywh.astype(np.float64), g_box, crowd).reshape(-1))


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
E2E_SIZE = 512
E2E_IMAGES = 2


@pytest.fixture(scope="module")
def small_tree(tmp_path_factory):
    """One R50 checkpoint and two 512^2 images with label files (both the test split)."""
    from deepemia_amd import synth

    root = tmp_path_factory.mktemp("evalcrops")
    cfgdir = root / "cfg"
    (cfgdir / "datasets").mkdir(parents=True)
    split = root / "split_dir"
    base = {"bucket": None,
            "paths": {"split_dir": str(split), "category_json": str(root / "dataset_info.json"), "local_dataset_root": str(root)},
            "inference_settings": {"confidence_mode": "auto", "spatial_constraints": {"default": {"enabled": False}}},
            "l4_performance_optimizations": {"enable_parallel_mask_processing": True}}
    (cfgdir / "config.yaml").write_text(yaml.safe_dump(base, sort_keys=False))
    (root / "dataset_info.json").write_text(json.dumps({DATASET: [str(root / "imgs"), str(root / "labels"), CLASSES]}))
    sd = synth.random_d2_state_dict(50, len(CLASSES), seed=0, mask_bias=0.5, mask_gain=6.0)
    mdir = split / DATASET / "rcnn_r50"
    mdir.mkdir(parents=True)
    synth.save_d2_checkpoint(str(mdir / "model_final_r50.pth"), sd)
    for d in (root / "imgs", root / "labels"):
        d.mkdir(parents=True)
    rng = np.random.RandomState(9)
    for i in range(E2E_IMAGES):
        name = f"em_{i}.png"
        Image.fromarray(synth.em_tile(70 + i, E2E_SIZE)[:, :, ::-1]).save(root / "imgs" / name, compress_level=1)
        lab = json.dumps(_labels(rng, name, E2E_SIZE))
        (root / "imgs" / f"em_{i}.json").write_text(lab)
        (root / "labels" / f"em_{i}.json").write_text(lab)
    return root, cfgdir, split


def _e2e_cfg(mask_frame, score_frame):
    inf = {"confidence_mode": "manual", "mask_frame": mask_frame,
           "class_specific_settings": {"class_0": {"confidence_threshold": 0.3, "iou_threshold": 0.6, "min_size": 25},
                                       "class_1": {"confidence_threshold": 0.35, "iou_threshold": 0.5, "min_size": 5}},
           "tile_settings": {"tile_size": 256, "overlap_ratio": 0.0, "upscale_factor": 1.0, "edge_filter_enabled": True},
           "ensemble_settings": {"enabled": False, "small_classes_only": False}}
    return {"inference_overrides": inf, "spatial_constraints": {"enabled": False},
            "evaluation": {"mode": "pipeline", "max_dets": [1, 10, 1000], "score_frame": score_frame}}


def test_evaluate_pipeline_mode_on_crops_end_to_end(small_tree, monkeypatch):
    """``evaluate_model(..., mode="pipeline")`` under ``crop_direct`` / ``crops`` writes what ``full`` / ``planes`` writes, byte
    for byte; the metrics are ``coco_ref``'s COCOeval on the written detections (to 1e-12, as the existing CLI test);
    ``crop`` / ``planes`` is refused."""
    from deepemia_amd.data.datasets import ellipse_polygon
    from deepemia_amd.functions.evaluate_model import evaluate_model
    from deepemia_amd.utils import config as C

    root, cfgdir, split = small_tree
    names = sorted(f"em_{i}.png" for i in range(E2E_IMAGES))
    try:
        outs = {}
        for mask_frame, score_frame in (("full", "planes"), ("crop_direct", "crops")):
            _configure(monkeypatch, small_tree, _e2e_cfg(mask_frame, score_frame), names)
            outs[score_frame] = evaluate_model(DATASET, str(root / score_frame), rcnn=50, mode="pipeline", threshold=0.3)
        for f in ("metrics.csv", "coco_instances_results.json"):
            assert _sha(root / "planes" / f) == _sha(root / "crops" / f), f
        a = torch.load(root / "planes" / "instances_predictions.pth", weights_only=False)
        b = torch.load(root / "crops" / "instances_predictions.pth", weights_only=False)
        assert a == b and [p["image_id"] for p in b] == list(range(E2E_IMAGES))
        res = json.loads((root / "crops" / "coco_instances_results.json").read_text())
        assert len(res) >= E2E_IMAGES and sorted({r["image_id"] for r in res}) == list(range(E2E_IMAGES))
        images, gts = R.gt_from_label_files(str(root / "labels"), [n.replace(".png", ".json") for n in names], CLASSES, ellipse_polygon)
        got = _metrics(root / "crops")
        for task in ("bbox", "segm"):
            stats, prec = X.coco_eval(images, gts, res, [0, 1], task, [1, 10, 1000])
            _same(got[task], R.derive(stats, prec, CLASSES))
            _same(outs["crops"][task], got[task])
        _configure(monkeypatch, small_tree, _e2e_cfg("crop", "planes"), names)
        with pytest.raises(ValueError, match="mask_frame: crop is not supported by the evaluate task"):
            evaluate_model(DATASET, str(root / "refused"), rcnn=50, mode="pipeline", threshold=0.3)
    finally:
        C.reset_cache()
