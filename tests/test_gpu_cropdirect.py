"""``mask_frame: crop_direct``: the contour trace, the measurements and the gray histogram of a crop-framed set on its words in
place (``CropMaskSet.trace`` / ``contours`` / ``gray_histogram``; ``demia_crop_contours_wl``, ``demia_crop_gray_histogram``) against the
plane kernels they are the twins of.  The same operations run in the same order on the same bits, so every comparison is exact.

Boxes are (y0, x0, y1, x1) everywhere, as in the C ABI."""
import numpy as np
import pytest
import torch

from test_gpu_cropset import _blob_planes, _fake_pipe, _set_frame, _write_tree

pytestmark = pytest.mark.gpu

H, W = 320, 1000          # W is no multiple of 32: 32 words per row, 8 bits of the last one used
TRACE_WORDS_SMALL, TRACE_WORDS = 1024, 8192
UM = 0.37


@pytest.fixture(scope="module")
def ops(gpu_device):
    from deepemia_amd.maskset import MaskOps
    return MaskOps(gpu_device)


def _ellipse(y0, x0, y1, x1):
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx, ry, rx = (y0 + y1) / 2, (x0 + x1) / 2, (y1 - y0) / 2 + 0.3, (x1 - x0) / 2 + 0.3
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0


def _masks() -> np.ndarray:
    """The masks of the trace tests; the two whose padded region exceeds the large LDS buffer are masks 10 and the LAST one."""
    z = lambda: np.zeros((H, W), bool)
    m = [z()]                                                                    # 0 empty
    a = z(); a[0, 0] = True; m.append(a)                                         # 1 single pixel in the frame's first corner
    a = z(); a[H - 1, W - 1] = True; m.append(a)                                 # 2 ... and in its last
    a = z(); a[50, 100:401] = True; m.append(a)                                  # 3 one row
    a = z(); a[20:301, 517] = True; m.append(a)                                  # 4 one column
    a = _ellipse(100, -20, 160, 40); m.append(a)                                 # 5 touches the left frame edge
    a = _ellipse(30, 950, 90, W + 15); a[40:60, 990:] = True; m.append(a)        # 6 touches the right frame edge
    a = z(); a[200:260, 300:360] = True; a[210:250, 310:350] = False; a[225:235, 325:335] = True; m.append(a)   # 7 ring, island in its hole
    a = _ellipse(10, 600, 40, 660) | _ellipse(25, 670, 70, 700); m.append(a)     # 8 two components
    a = _ellipse(110, 400, 209, 699); a[150:170, 500:600] = False; m.append(a)   # 9 100 x 300 px: the list kernel's LDS path
    a = _ellipse(10, 20, 309, 979)                                               # 10 300 x 960 px: beyond the large LDS buffer, with
    a[100:140, 300:420] = False; a[180:230, 600:640] = False                     #    two holes,
    a[110:130, 340:380] = True                                                   #    an island in one of them (skipped: RETR_EXTERNAL)
    a[12:20, 24:40] = True; m.append(a)                                          #    and a second component in the box's corner
    g = np.random.default_rng(5)
    for _ in range(12):                                                          # 11 .. 22 blobs of all sizes
        bh, bw = int(g.integers(2, 90)), int(g.integers(2, 200))
        y0, x0 = int(g.integers(0, H - bh)), int(g.integers(0, W - bw))
        m.append(_ellipse(y0, x0, y0 + bh - 1, x0 + bw - 1))
    m.append(_ellipse(8, 30, 311, 995))                                          # 23 beyond the large LDS buffer, stored LAST
    return np.stack(m)


def _set_with_rooms(ops, dense, grow):
    """dense masks -> (CropMaskSet whose rooms are the tight boxes grown by ``grow`` [n, 4] pixels per side and clipped, planes)."""
    from deepemia_amd.cropset import CropMaskSet
    ops.set_frame_width(W)
    planes = ops.from_dense(dense).contiguous()
    area, bbox = ops.area_bbox(planes)
    bb = bbox.cpu().numpy()
    room = bb.copy()
    room[:, 0] = np.maximum(bb[:, 0] - grow[:, 0], 0); room[:, 1] = np.maximum(bb[:, 1] - grow[:, 1], 0)
    room[:, 2] = np.minimum(bb[:, 2] + grow[:, 2], H - 1); room[:, 3] = np.minimum(bb[:, 3] + grow[:, 3], W - 1)
    room[bb[:, 0] < 0] = -1
    cs = CropMaskSet.from_planes(ops, planes, W, bbox=room, area=area.cpu().numpy())
    cs.bbox = bbox                                                               # the TIGHT boxes, as the contract has them
    return cs, planes


def _padded_region_words(box):
    """(rh + 2) * (rw + 2) of a box's region: grown by one ring, clipped to the frame, on the word grid."""
    box = np.asarray(box, dtype=np.int64).reshape(-1, 4)
    rh = np.minimum(box[:, 2] + 1, H - 1) - np.maximum(box[:, 0] - 1, 0) + 1
    rw = (np.minimum(box[:, 3] + 1, W - 1) >> 5) - (np.maximum(box[:, 1] - 1, 0) >> 5) + 1
    return np.where(box[:, 0] >= 0, (rh + 2) * (rw + 2), 0)


@pytest.fixture(scope="module")
def env(ops):
    dense = _masks()
    n = len(dense)
    g = np.random.default_rng(6)
    grow = g.integers(0, 38, size=(n, 4))
    grow[::3] = 0                                                                # every third room IS its tight box: the ring lies outside it
    grow[10] = (0, 5, 3, 0)
    cs, planes = _set_with_rooms(ops, dense, grow)
    from oracle import postproc_ref as P
    ref = [P.find_external_contours(d) for d in dense]                           # computed once, shared, never changed
    return dict(dense=dense, cs=cs, planes=planes, ref=ref, n=n)


def _measured(cset, um=UM):
    cset.launch_measure(um, slots=4)
    cset.fetch(with_points=True)
    return cset


def _assert_same_contours(ops, cs, planes, ref=None, **trace_kw):
    """``cs.trace`` against ``ops.trace`` of the same masks as planes: counts, then per mask points, area, perimeter and the 12
    values, all exact; ``ref``: the oracle's contours per mask as well.  Returns the crop-framed ContourSet."""
    ops.set_frame_width(W)
    a = _measured(cs.trace(max_contours=256, **trace_kw))
    b = _measured(ops.trace(planes, max_contours=256, bbox=cs.bbox))
    assert int(a.counters[1].item()) == 0 and int(b.counters[1].item()) == 0     # no error bit
    assert np.array_equal(a.host()[0], b.host()[0])                              # count
    ra, rb = a.records(um_pix=UM, measure=True), b.records(um_pix=UM, measure=True)
    for i, (qa, qb) in enumerate(zip(ra, rb)):
        assert len(qa) == len(qb), i
        for x, y in zip(qa, qb):
            np.testing.assert_array_equal(x["points"], y["points"])
            assert x["area"] == y["area"] and x["perimeter"] == y["perimeter"], i
            assert all(float(u) == float(v) or (np.isnan(u) and np.isnan(v)) for u, v in zip(x["values"], y["values"])), (i, x["values"], y["values"])
        if ref is not None:
            assert len(qa) == len(ref[i]), (i, len(qa), len(ref[i]))
            for x, c in zip(qa, ref[i]):
                np.testing.assert_array_equal(x["points"], c)
    return a


# ------------------------------------------------------------------------------------------------------------------- trace
def test_trace_equals_the_plane_kernel_table_for_table(ops, env):
    cs, n = env["cs"], env["n"]
    assert n == 24 and len(env["ref"][0]) == 0 and len(env["ref"][7]) == 1 and len(env["ref"][8]) == 2 and len(env["ref"][10]) == 2
    bb = cs.bbox.cpu().numpy()
    pn = _padded_region_words(bb)
    assert TRACE_WORDS_SMALL < pn[9] <= TRACE_WORDS and pn[10] > TRACE_WORDS and pn[n - 1] > TRACE_WORDS      # all three kernels' paths
    assert (pn[:9] <= TRACE_WORDS_SMALL).all() and bb[5, 1] == 0 and bb[6, 3] == W - 1
    assert np.array_equal(cs.room_h[::3][1:], bb[::3][1:]) and cs.offsets_h[n - 1] == cs.offsets_h.max()       # tight rooms; a large mask last
    a = _assert_same_contours(ops, cs, env["planes"], env["ref"])
    assert a.walker_stats[0] > 0                                                  # some masks took the parallel walkers


def test_ring_words_are_never_fetched_from_the_payload(ops, env):
    """Every room equals its tight box, so every ring row and ring word column lies outside its room; the masks alternate with
    solid word-aligned blocks of ones, so the words before and behind a mask's own are all ones, and the payload is a view of a
    buffer that goes on with 4096 words of ones.  Catches the variant that copies the region out of ``payload`` with the room's
    stride but without the in-room test (a room addressed like a plane): it reads the neighbour's ones as the row above / below a
    mask and the mask's own next row as its right ring word, the top row stops being a border, and the contours differ from the
    twin's (which traces planes that are zero there)."""
    dense = env["dense"]
    solid = np.zeros((H, W), bool); solid[100:110, 320:448] = True               # 10 rows x 4 whole words of ones
    order, ref = [], []
    for i in range(len(dense)):
        order += [solid, dense[i]]
        ref += [None, env["ref"][i]]
    order.append(solid)
    ref.append(None)
    inter = np.stack(order)
    cs, planes = _set_with_rooms(ops, inter, np.zeros((len(inter), 4), dtype=np.int64))
    assert np.array_equal(cs.room_h, cs.bbox.cpu().numpy())
    pay = cs.payload[:cs.words].cpu().numpy().view(np.uint32)
    assert (pay[:40] == 0xFFFFFFFF).all() and (pay[-40:] == 0xFFFFFFFF).all()
    buf = torch.full((cs.words + 4096,), -1, dtype=torch.int32, device=ops.device)
    buf[:cs.words] = cs.payload[:cs.words]
    cs.payload = buf[:cs.words]
    from oracle import postproc_ref as P
    ref_solid = P.find_external_contours(solid)
    _assert_same_contours(ops, cs, planes, [ref_solid if r is None else r for r in ref])
    assert bool((buf[cs.words:] == -1).all())


def test_scratch_stays_room_sized(ops, env):
    """Only the two masks beyond the large LDS buffer get scratch, at most two padded regions of their ROOM each; a canary behind
    exactly that many words survives the trace, and trace + measure + fetch allocate less than M full-frame planes.

    The pools of this test are sized to the set: ``max_contours`` 8 and a point pool of the oracle's own point count (+ the 4 spare
    slots per contour, rounded up to 1024).  The default pools -- 256 contour slots per mask, 4096 points per mask + 65536 -- are
    sized for the thousands of masks of a large image, are the same in every frame, and alone exceed 24 planes of 320 x 32 words."""
    cs, n = env["cs"], env["n"]
    off, total = cs.contour_scratch()
    lens = np.diff(np.concatenate((off, [total])))
    big = [10, n - 1]
    assert (np.delete(lens, big) == 0).all() and (lens[big] > 0).all()
    assert (lens[big] <= 2 * _padded_region_words(cs.room_h[big])).all()
    need = sum(len(c) + 4 for r in env["ref"] for c in r)
    mp = (need + 1023) // 1024 * 1024
    canary = 0x5A5A5A5A
    scratch = torch.full((total + 1024,), canary, dtype=torch.int32, device=ops.device)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a = cs.trace(max_contours=8, max_points=mp, scratch=scratch)
    _measured(a)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    planes_bytes = n * H * ((W + 31) // 32) * 4
    print(f"trace + measure + fetch allocated {peak} bytes at most; {n} full-frame planes are {planes_bytes} bytes; scratch {4 * total} bytes")
    assert bool((scratch[total:] == canary).all())
    assert int(a.counters[1].item()) == 0 and int(a.host()[0].sum()) == sum(len(r) for r in env["ref"])
    assert peak < planes_bytes


# --------------------------------------------------------------------------------------------------------------- histogram
@pytest.mark.parametrize("channels", [3, 1])
def test_gray_histogram_equals_the_plane_kernel(ops, env, channels):
    cs, dense = env["cs"], env["dense"]
    g = np.random.default_rng(9)
    img = g.integers(0, 256, size=(H, W, 3) if channels == 3 else (H, W), dtype=np.uint8)
    image = torch.from_numpy(img).to(ops.device)
    ops.set_frame_width(W)
    got = cs.gray_histogram(image)
    assert got.shape == (len(dense), 256) and np.array_equal(got, ops.gray_histogram(env["planes"], image, bbox=cs.bbox))
    assert np.array_equal(got.sum(axis=1), dense.sum(axis=(1, 2)))
    if channels == 1:
        for i, d in enumerate(dense):
            assert np.array_equal(got[i], np.bincount(img[d], minlength=256)), i


# ------------------------------------------------------------------------------------------------------------------- waits
def test_waits_of_the_merge_do_not_grow_with_the_instance_count(gpu_device):
    from deepemia_amd.cropset import CropMaskSet, rooms_of_placed_tiles
    h = w = 512
    tile = 128
    pipes = {f: _fake_pipe(gpu_device, f) for f in ("full", "crop", "crop_direct")}
    waits, kept = {}, {}
    for n in (20, 60):
        half = _blob_planes(pipes["full"].ops, n // 2, tile, tile, 41 + n, max_box=40, dup=False)
        src = torch.cat([half, half]).contiguous()                               # every mask twice at the same place: the merge removes some
        pipes["full"].ops.set_frame_width(tile)
        _, sbb = pipes["full"].ops.area_bbox(src)
        sbb = sbb.cpu().numpy()
        g = np.random.default_rng(42)
        xo, yo = 2 * (g.integers(0, 5, n // 2) * 96).tolist(), 2 * (g.integers(0, 5, n // 2) * 96).tolist()
        scores, classes = (g.permutation(n) / n).tolist(), [0] * n
        for frame, pipe in pipes.items():
            pipe.ops.set_frame_width(w)
            if frame == "full":
                placed = pipe.ops.place_tiles(src, xo, yo, tile, tile, h, w, src_w=tile)
            else:
                placed = CropMaskSet.place_tiles(pipe.ops, src, rooms_of_placed_tiles(sbb, (tile, tile), (tile, tile), xo, yo, (h, w)), xo, yo,
                                                 tile, tile, h, w, src_w=tile)
            w0 = pipe.d2h_waits
            m, s, c = pipe.deduplicate_masks_smart(placed, scores, classes, 0.4)
            waits[frame, n] = pipe.d2h_waits - w0
            kept[frame, n] = (m if frame == "full" else m.to_planes(), s, c)
        for frame in ("crop", "crop_direct"):
            assert kept[frame, n][1:] == kept["full", n][1:] and torch.equal(kept[frame, n][0], kept["full", n][0])
        assert 0 < len(kept["full", n][1]) < n
    assert waits["crop_direct", 20] == waits["crop_direct", 60] == waits["full", 60]
    assert waits["crop", 60] >= -(-60 // 16) > waits["crop_direct", 60]
    st = pipes["crop_direct"].end_image_stats((h, w))
    assert st["full_frame_planes_peak"] == 0 and st["plane_pool_capacity"] == 0
    assert "_crop_planes" not in pipes["crop_direct"].ops.__dict__             # no pool was ever made


# --------------------------------------------------------------------------------------------------------------------- CLI
@pytest.mark.parametrize("upscale", [1.0, 2.0])
def test_cli_writes_the_same_bytes_with_crop_direct(tmp_path, monkeypatch, gpu_device, upscale):
    import main as cli
    from deepemia_amd.functions import inference as inf_mod
    from deepemia_amd.utils import config as C
    from test_gpu_cropset import DATASET

    ds_cfg = {"inference_overrides": {"confidence_mode": "manual",
                                      "class_specific_settings": {"class_0": {"confidence_threshold": 0.3, "iou_threshold": 0.6},
                                                                  "class_1": {"confidence_threshold": 0.35, "iou_threshold": 0.5}},
                                      "tile_settings": {"tile_size": 200, "overlap_ratio": 0.125, "upscale_factor": upscale, "edge_filter_enabled": True},
                                      "spatial_constraints": {"enabled": True, "containment_rules": {1: 0}, "containment_threshold": 0.5}}}
    cfgdir, split = _write_tree(tmp_path, ds_cfg)                                # (its global config switches measure_contrast_distribution on)
    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(cfgdir))
    monkeypatch.setenv("DEEPEMIA_OFFLINE", "1")
    monkeypatch.setenv("DEEPEMIA_WORKERS", "1")
    monkeypatch.chdir(tmp_path)
    names = ["measurements_results.csv", "R50_flip_results.csv", "class_color_legend.txt", "em_0.tif_predictions.png", "em_1.tif_predictions.png"]
    outs, stats = {}, {}
    for frame in ("full", "crop_direct"):
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
        assert outs["crop_direct"][nm] == outs["full"][nm], nm
    st = stats["crop_direct"]
    assert st["mask_frame"] == "crop_direct" and st["full_frame_planes_peak"] == 0 and st["plane_pool_capacity"] == 0
