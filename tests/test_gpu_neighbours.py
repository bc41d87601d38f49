"""``demia_mask_neighbours`` / ``demia_crop_neighbours`` -- nearest edge-to-edge gaps and contact counts between the masks of a frame
-- against the literal reference of ``tests/neighbour_ref.py`` on the scenes of ``tests/neighbour_cases.py`` and on seeded random
scenes, integer for integer; then the border points, crops against planes, position and order invariance, the bounds of every
output, the ride in ``ContourSet.fetch`` and the CLI in every mask frame and over two ranks."""
import csv
import io

import numpy as np
import pytest

import neighbour_cases as NC
import neighbour_ref as NR

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A
GUARD = 64                       # int32 words of canary on either side of every output
SCENES = NC.by_name()


@pytest.fixture(scope="module")
def ops(gpu_device):
    from deepemia_amd.maskset import MaskOps
    return MaskOps(gpu_device)


@pytest.fixture(scope="module")
def refs():
    """name -> (table, sums) of the reference, computed once and shared."""
    return {n: (NR.table(s.masks, s.group, s.r2), NR.sums(s.masks)) for n, s in SCENES.items()}


def _planes(ops, masks):
    ops.set_frame_width(masks.shape[2])
    return ops.from_dense(masks)


def _run_planes(ops, s):
    return ops.neighbours(_planes(ops, s.masks), None, None, group=s.group, r2=s.r2)


def _crops(ops, masks, grow=None, seed=0):
    """The scene as a crop-framed set: rooms = tight boxes, or grown by up to ``grow`` pixels per side (clipped to the frame)."""
    from deepemia_amd.cropset import CropMaskSet
    H, W = masks.shape[1:]
    cs = CropMaskSet.from_planes(ops, _planes(ops, masks), W)
    if grow:
        rng = np.random.default_rng(seed)
        room = cs.room_h.copy()
        for r in room:
            if r[0] >= 0:
                g = rng.integers(0, grow + 1, 4)
                r[:] = (max(r[0] - g[0], 0), max(r[1] - g[1], 0), min(r[2] + g[2], H - 1), min(r[3] + g[3], W - 1))
        cs = cs.reroom(room)
    return cs


def _host(nb):
    return nb.table.cpu().numpy().tolist(), nb.sums.cpu().numpy().tolist()


def _check_points(nb, masks):
    pts, nbd, off = nb.points.cpu().numpy().view(np.uint32), nb.nborder.cpu().numpy(), nb.point_off
    for m in range(masks.shape[0]):
        want = NR.border(masks[m])
        got = pts[off[m]: off[m] + nbd[m]]
        assert int(nbd[m]) == len(want) <= off[m + 1] - off[m], m
        assert set(zip((got >> 16).tolist(), (got & 0xffff).tolist())) == want, m


# ------------------------------------------------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("name", list(SCENES))
def test_both_entries_equal_the_reference(ops, refs, name):
    s = SCENES[name]
    want_t, want_s = refs[name]
    nb = _run_planes(ops, s)
    got_t, got_s = _host(nb)
    assert got_s == want_s
    bad = [(a, g, w) for a, (g, w) in enumerate(zip(got_t, want_t)) if g != w]
    assert not bad, bad[:5]
    _check_points(nb, s.masks)
    cs = _crops(ops, s.masks)
    nc = cs.neighbours(group=s.group, r2=s.r2)
    assert _host(nc) == (want_t, want_s)
    _check_points(nc, s.masks)


def test_random_scenes_equal_the_reference(ops):
    for seed in NC.RANDOM_SEEDS:
        s = NC.random_scene(seed)
        want = (NR.table(s.masks, s.group, s.r2), NR.sums(s.masks))
        nb = _run_planes(ops, s)
        assert _host(nb) == want, seed
        nc = _crops(ops, s.masks, grow=40 if seed % 2 else None, seed=seed).neighbours(group=s.group, r2=s.r2)
        assert _host(nc) == want, seed
        if seed % 8 == 0:
            _check_points(nb, s.masks)
            _check_points(nc, s.masks)


def test_without_groups_the_group_columns_repeat_the_nearest(ops):
    s = SCENES["groups_differ"]
    t, _ = _host(ops.neighbours(_planes(ops, s.masks), None, None, group=None, r2=-1))
    assert t == NR.table(s.masks, None, -1) and all(r[0:2] == r[2:4] and r[5] == -1 for r in t)


# ------------------------------------------------------------------------------------------------------- 2. crops against planes
@pytest.mark.parametrize("name", ["overlap_contained", "disc_in_hole", "edges_corners", "empty_among", "interlocking_ls", "combs"])
def test_crops_equal_planes_in_tight_and_grown_rooms(ops, name):
    import torch
    s = SCENES[name]
    nb = _run_planes(ops, s)
    for grow, seed in ((None, 0), (40, 1), (40, 2), (7, 3)):
        nc = _crops(ops, s.masks, grow=grow, seed=seed).neighbours(group=s.group, r2=s.r2)
        assert torch.equal(nc.table, nb.table) and torch.equal(nc.sums, nb.sums) and torch.equal(nc.nborder, nb.nborder), (grow, seed)


def test_selected_subset_equals_the_reference_on_that_subset(ops):
    for seed in (5, 11, 24):
        s = NC.random_scene(seed)
        M = s.masks.shape[0]
        rng = np.random.default_rng(seed)
        idx = rng.permutation(M)[: max(2, M // 2)]
        sub = _crops(ops, s.masks, grow=12, seed=seed).select(idx)
        got = _host(sub.neighbours(group=s.group[idx], r2=s.r2))
        assert got == (NR.table(s.masks[idx], s.group[idx], s.r2), NR.sums(s.masks[idx])), seed


# ------------------------------------------------------------------------------------------------------- 3. invariance
def test_translation_by_33_17(ops):
    for seed in (1, 2, 3):
        s = NC.random_scene(seed)
        M, H, W = s.masks.shape
        a = np.zeros((M, H + 30, W + 45), dtype=bool)
        b = np.zeros_like(a)
        a[:, :H, :W] = s.masks
        b[:, 17:17 + H, 33:33 + W] = s.masks
        ta, sa = _host(ops.neighbours(_planes(ops, a), None, None, group=s.group, r2=s.r2))
        tb, sb = _host(ops.neighbours(_planes(ops, b), None, None, group=s.group, r2=s.r2))
        assert ta == tb == NR.table(s.masks, s.group, s.r2)
        assert [[n, sx + 33 * n, sy + 17 * n] for n, sx, sy in sa] == sb


def test_permutation_of_the_masks(ops):
    for name in ("tie_lower_index_wins", "tie_symmetric", "many_small"):
        s = SCENES[name]
        M = s.masks.shape[0]
        group = s.group if s.group is not None else np.zeros(M, dtype=np.int32)
        perm = np.random.default_rng(7).permutation(M)
        t0, s0 = _host(ops.neighbours(_planes(ops, s.masks), None, None, group=group, r2=s.r2))
        t1, s1 = _host(ops.neighbours(_planes(ops, s.masks[perm]), None, None, group=group[perm], r2=s.r2))
        assert t1 == NR.table(s.masks[perm], group[perm], s.r2)                  # ties go to the lower index of the NEW order
        for i, p in enumerate(perm.tolist()):
            assert s1[i] == s0[p]
            assert [t1[i][c] for c in (0, 2, 4, 5)] == [t0[p][c] for c in (0, 2, 4, 5)]      # distances and counts move with their mask


# ------------------------------------------------------------------------------------------------------- 4. bounds
@pytest.mark.parametrize("name", ["edges_corners", "empty_among", "many_small", "combs"])
@pytest.mark.parametrize("frame", ["planes", "crops"])
def test_nothing_is_written_outside_the_outputs(ops, refs, name, frame):
    """Every output of the C entries carved out of one canary buffer: only points[0 .. point_off[M]), nborder, sums and table
    change -- and of the points only each mask's first nborder."""
    import torch

    from deepemia_amd import _lib
    from deepemia_amd.maskset import neighbour_offsets
    s = SCENES[name]
    M, H, W = s.masks.shape
    area = s.masks.reshape(M, -1).sum(1)
    off = neighbour_offsets(area)
    total = int(off[-1])
    sizes = [total + (total & 1), M + (M & 1), 2 * 3 * M, 2 * 6 * M]              # int32 words; even, so the int64 tables stay aligned
    flat = torch.from_numpy(np.full(sum(sizes) + GUARD * (len(sizes) + 1), CANARY, dtype=np.uint32).view(np.int32)).to(ops.device)
    views, pos = [], GUARD
    for n in sizes:
        views.append(flat[pos:pos + n])
        pos += n + GUARD
    points, nborder, sums, table = views
    off_d = ops.upload(off)
    group_d = None if s.group is None else ops.upload(s.group)
    planes = _planes(ops, s.masks)
    bbox = ops.upload(NR.tight_boxes(s.masks))
    if frame == "planes":
        st = ops.lib.demia_mask_neighbours(_lib.ptr(planes), _lib.ptr(bbox), _lib.ptr(group_d), M, H, W, s.r2, _lib.ptr(off_d), _lib.ptr(points),
                                           _lib.ptr(nborder), _lib.ptr(sums), _lib.ptr(table), ops._stream())
    else:
        cs = _crops(ops, s.masks, grow=9, seed=4)
        st = ops.lib.demia_crop_neighbours(_lib.ptr(cs.payload), _lib.ptr(cs.room), _lib.ptr(cs.offsets), _lib.ptr(cs.bbox), _lib.ptr(group_d), M, H, W,
                                           s.r2, _lib.ptr(off_d), _lib.ptr(points), _lib.ptr(nborder), _lib.ptr(sums), _lib.ptr(table), ops._stream())
    _lib.check(st, "neighbours")
    host = flat.cpu().numpy().view(np.uint32)
    keep = np.ones(host.shape, dtype=bool)
    pos = GUARD
    for n in sizes:
        keep[pos:pos + n] = False
        pos += n + GUARD
    assert (host[keep] == CANARY).all()
    nb_h = nborder.cpu().numpy()[:M]
    pts = points.cpu().numpy().view(np.uint32)
    for m in range(M):
        assert (pts[off[m] + nb_h[m]: off[m + 1]] == CANARY).all(), m
    want_t, want_s = refs[name]
    assert table.view(torch.int64).view(M, 6).cpu().numpy().tolist() == want_t
    assert sums.view(torch.int64).view(M, 3).cpu().numpy().tolist() == want_s


def test_no_masks_and_bad_arguments(ops):
    import torch

    from deepemia_amd import _lib
    t = torch.zeros((8,), dtype=torch.int64, device=ops.device)
    p = _lib.ptr(t)
    assert ops.lib.demia_mask_neighbours(0, 0, 0, 0, 40, 70, -1, 0, 0, 0, 0, 0, ops._stream()) == 0
    assert ops.lib.demia_crop_neighbours(0, 0, 0, 0, 0, 0, 40, 70, -1, 0, 0, 0, 0, 0, ops._stream()) == 0
    for H, W in ((0, 70), (40, 0), (65536, 70), (40, 65536)):
        assert ops.lib.demia_mask_neighbours(p, p, 0, 1, H, W, -1, p, p, p, p, p, ops._stream()) != 0
    assert ops.lib.demia_mask_neighbours(p, p, 0, -1, 40, 70, -1, p, p, p, p, p, ops._stream()) != 0
    assert ops.lib.demia_mask_neighbours(p, p, 0, 1, 40, 70, -1, p, 0, p, p, p, ops._stream()) != 0
    assert ops.lib.demia_crop_neighbours(p, 0, p, p, 0, 1, 40, 70, -1, p, p, p, p, p, ops._stream()) != 0
    with pytest.raises(_lib.HipKernelError, match="demia_mask_neighbours"):
        _lib.check(ops.lib.demia_mask_neighbours(0, p, 0, 1, 40, 70, -1, p, p, p, p, p, ops._stream()), "demia_mask_neighbours")
    from deepemia_amd.cropset import CropMaskSet
    empty = np.zeros((0, 40, 70), dtype=bool)
    nb = ops.neighbours(_planes(ops, empty), None, None)
    assert tuple(nb.table.shape) == (0, 6) and tuple(nb.sums.shape) == (0, 3) and nb.point_off.tolist() == [0]
    nc = CropMaskSet.empty(ops, (40, 70)).neighbours()
    assert tuple(nc.table.shape) == (0, 6)


def test_a_short_point_share_is_cut_not_overrun(ops):
    """``area`` sizes the shares; one that is too small for a mask's border cuts that mask's points to its share."""
    s = SCENES["overlap_contained"]
    area = s.masks.reshape(4, -1).sum(1).astype(np.int64)
    want = [len(NR.border(m)) for m in s.masks]
    area[0] = 10
    planes = _planes(ops, s.masks)
    nb = ops.neighbours(planes, ops.upload(NR.tight_boxes(s.masks)), area, r2=-1)
    assert nb.nborder.cpu().numpy().tolist() == want and nb.point_off.tolist() == [0, 10, 10 + area[1], 10 + area[1] + area[2], area.sum()]
    pts = nb.points.cpu().numpy().view(np.uint32)
    for m in (1, 2, 3):                                                          # the neighbours' shares are untouched by mask 0's overflow
        got = pts[nb.point_off[m]: nb.point_off[m] + want[m]]
        assert set(zip((got >> 16).tolist(), (got & 0xffff).tolist())) == NR.border(s.masks[m])
    assert nb.sums.cpu().numpy().tolist() == NR.sums(s.masks)


# ------------------------------------------------------------------------------------------------------- 5. the ride in the fetch
@pytest.mark.parametrize("frame", ["planes", "crops"])
def test_tables_ride_in_the_contour_fetch(ops, monkeypatch, frame):
    import torch

    from deepemia_amd.maskset import Neighbours
    s = NC.random_scene(9)
    masks = s.masks[[k for k in range(len(s.masks)) if s.masks[k].any()]]
    group = np.arange(len(masks), dtype=np.int32) % 2
    planes = _planes(ops, masks)
    area = masks.reshape(len(masks), -1).sum(1)
    bbox = ops.upload(NR.tight_boxes(masks))
    alone = _host(ops.neighbours(planes, bbox, area, group=group, r2=30))
    if frame == "planes":
        cs = ops.trace(planes, max_contours=64, bbox=bbox, total_area=int(area.sum()))
        nb = ops.neighbours(planes, bbox, area, group=group, r2=30)
    else:
        cset = _crops(ops, masks, grow=5)
        cs = cset.trace(max_contours=64, total_area=int(area.sum()))
        nb = cset.neighbours(area=area, group=group, r2=30)
    cs.launch_measure(1.0, slots=4)
    copies = [0]
    cpu = torch.Tensor.cpu

    def spy(self, *a, **k):
        copies[0] += 1
        return cpu(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "cpu", spy)
    got = cs.fetch(extra=[nb.table_i32, nb.sums_i32], with_points=True)
    monkeypatch.undo()
    assert copies[0] == 1                                                        # the one copy of the fetch brought the tables too
    t, sm = Neighbours.from_i32(got[-2], got[-1])
    assert (t.tolist(), sm.tolist()) == alone == (NR.table(masks, group, 30), NR.sums(masks))


# ------------------------------------------------------------------------------------------------------- 6. CLI
RADIUS = 9.5


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory, gpu_device):
    """``main.py --task inference`` on two small images, once per (mask frame, setting): the output files of every run, the
    pipeline's ``d2h_waits`` and the device-to-host copies it made."""
    import torch

    import main as cli
    from deepemia_amd.functions import inference as inf_mod
    from deepemia_amd.utils import config as C
    from test_gpu_cropset import DATASET, _set_frame, _write_tree

    tmp_path = tmp_path_factory.mktemp("neighbours_cli")
    ds_cfg = {"inference_overrides": {"confidence_mode": "manual",
                                      "class_specific_settings": {"class_0": {"confidence_threshold": 0.3, "iou_threshold": 0.6},
                                                                  "class_1": {"confidence_threshold": 0.35, "iou_threshold": 0.5}},
                                      "tile_settings": {"tile_size": 200, "overlap_ratio": 0.125, "upscale_factor": 1.0, "edge_filter_enabled": True},
                                      "spatial_constraints": {"enabled": True, "containment_rules": {1: 0}, "containment_threshold": 0.5}}}
    on, on_r = {"neighbour_statistics": True}, {"neighbour_statistics": True, "neighbour_radius": RADIUS}
    runs = (("full", "off", {}), ("full", "on", on), ("crop", "off", {}), ("crop", "on", on), ("crop_direct", "off", {}), ("crop_direct", "on", on),
            ("full", "radius", on_r), ("crop_direct", "radius", on_r))
    names = ["measurements_results.csv", "R50_flip_results.csv", "neighbours_results.csv"]
    outs = {}
    with pytest.MonkeyPatch.context() as mp:
        cfgdir, split = _write_tree(tmp_path, ds_cfg)
        mp.setenv("DEEPEMIA_CONFIG_DIR", str(cfgdir))
        mp.setenv("DEEPEMIA_OFFLINE", "1")
        mp.setenv("DEEPEMIA_WORKERS", "1")
        mp.chdir(tmp_path)
        pipes, copies = [], [0]
        init, cpu = inf_mod.InferencePipeline.__init__, torch.Tensor.cpu

        def spy_init(self, *a, **k):
            init(self, *a, **k)
            pipes.append(self)

        def spy_cpu(self, *a, **k):
            copies[0] += 1
            return cpu(self, *a, **k)
        mp.setattr(inf_mod.InferencePipeline, "__init__", spy_init)
        mp.setattr(torch.Tensor, "cpu", spy_cpu)
        for frame, label, extra in runs:
            _set_frame(cfgdir, {"inference_overrides": dict(ds_cfg["inference_overrides"], **extra)}, frame)
            C.reset_cache()
            del pipes[:]
            copies[0] = 0
            assert cli.main(["--task", "inference", "--dataset_name", DATASET, "--threshold", "0.3", "--no-gpu-check"]) == 0
            C.reset_cache()
            files = {nm: (split / nm).read_bytes() if (split / nm).exists() else None for nm in names}
            outs[frame, label] = dict(files=files, d2h_waits=pipes[-1].d2h_waits, copies=copies[0])
            for nm in names:
                if (split / nm).exists():
                    (split / nm).unlink()
    return outs


def test_cli_setting_off_writes_no_file_and_on_changes_no_other_byte(cli_runs):
    for frame in ("full", "crop", "crop_direct"):
        off, on = cli_runs[frame, "off"]["files"], cli_runs[frame, "on"]["files"]
        assert off["neighbours_results.csv"] is None and on["neighbours_results.csv"] is not None, frame
        for nm in ("measurements_results.csv", "R50_flip_results.csv"):
            assert on[nm] == off[nm] and len(off[nm]) > 200, (frame, nm)
    for frame in ("full", "crop_direct"):
        for nm in ("measurements_results.csv", "R50_flip_results.csv"):
            assert cli_runs[frame, "radius"]["files"][nm] == cli_runs[frame, "off"]["files"][nm]


def test_cli_file_is_the_same_in_every_mask_frame(cli_runs):
    ref = cli_runs["full", "on"]["files"]["neighbours_results.csv"]
    for frame in ("crop", "crop_direct"):
        assert cli_runs[frame, "on"]["files"]["neighbours_results.csv"] == ref, frame
    assert cli_runs["crop_direct", "radius"]["files"]["neighbours_results.csv"] == cli_runs["full", "radius"]["files"]["neighbours_results.csv"]


def test_cli_adds_no_wait_and_no_copy(cli_runs):
    for frame in ("full", "crop", "crop_direct"):
        off, on = cli_runs[frame, "off"], cli_runs[frame, "on"]
        assert on["d2h_waits"] == off["d2h_waits"] > 0, frame
        assert on["copies"] == off["copies"] > 0, frame                          # the tables came in a copy that was made anyway
    assert cli_runs["full", "radius"]["d2h_waits"] == cli_runs["full", "off"]["d2h_waits"]


@pytest.mark.parametrize("label", ["on", "radius"])
def test_cli_values_equal_the_reference_on_the_masks_of_the_run(cli_runs, label):
    """The run's own ``R50_flip_results.csv`` decoded to dense masks, the reference on them, ``neighbour_rows`` on the reference's
    tables, ``csv.writer``: the bytes of ``neighbours_results.csv``."""
    from deepemia_amd.functions.inference import NEIGHBOUR_CSV_HEADER, neighbour_r2, neighbour_rows
    from test_gpu_cropset import CLASSES
    from test_gpu_pipeline_e2e import _rle_decode
    files = cli_runs["full", label]["files"]
    got = list(csv.reader(io.StringIO(files["neighbours_results.csv"].decode(), newline="")))
    assert got[0] == NEIGHBOUR_CSV_HEADER
    rle = list(csv.reader(io.StringIO(files["R50_flip_results.csv"].decode(), newline="")))[1:]
    meas = list(csv.reader(io.StringIO(files["measurements_results.csv"].decode(), newline="")))[1:]
    hw = {"em_0": (300, 417), "em_1": (260, 500)}
    r2 = neighbour_r2(RADIUS if label == "radius" else None, 1.0)
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(NEIGHBOUR_CSV_HEADER)
    seen = 0
    for image in [r[0] for k, r in enumerate(rle) if k == 0 or rle[k - 1][0] != r[0]]:         # the images in the file's order
        masks = np.stack([_rle_decode(r[1], *hw[image]) for r in rle if r[0] == image])
        mine = [r for r in got[1:] if r[13] == image + ".tif"]
        assert len(mine) == len(masks) >= 3 and [r[0] for r in mine] == [f"{image}.tif_{k + 1}" for k in range(len(masks))]
        classes = [int(r[1]) for r in mine]
        # (the ids and classes are the measurement file's: same k, same class)
        assert {r[0]: r[1] for r in meas if r[19] == image + ".tif"}.items() <= {r[0]: r[1] for r in mine}.items()
        for r in neighbour_rows(image + ".tif", classes, CLASSES, np.array(NR.table(masks, classes, r2), dtype=np.int64),
                                np.array(NR.sums(masks), dtype=np.int64), 1.0, "0"):
            w.writerow(r)
        seen += len(masks)
    assert seen == len(got) - 1 == len(rle)
    assert buf.getvalue().encode() == files["neighbours_results.csv"]
    within = [r[11] for r in got[1:]]
    assert all(v == "" for v in within) if label == "on" else (all(v != "" for v in within) and any(int(v) > 0 for v in within))


def test_cli_two_ranks_sharded_by_image_write_the_single_process_file(tmp_path, monkeypatch, gpu_device):
    import socket

    import torch.multiprocessing as mp

    from test_gpu_pipeline_e2e import _cli_rank_worker, _run_cli_plain, _write_tree
    tile = {"tile_size": 256, "overlap_ratio": 0.125, "upscale_factor": 1.0, "edge_filter_enabled": True}
    ds_cfg = {"inference_overrides": {"confidence_mode": "manual", "neighbour_statistics": True, "neighbour_radius": 12,
                                      "class_specific_settings": {"class_0": {"confidence_threshold": 0.3, "iou_threshold": 0.6},
                                                                  "class_1": {"confidence_threshold": 0.35, "iou_threshold": 0.5}},
                                      "tile_settings": tile, "spatial_constraints": {"enabled": True, "containment_rules": {1: 0}, "containment_threshold": 0.5}}}
    cfgdir, split, sds, images = _write_tree(tmp_path, [50], 0.5, 6.0, 5, 512, ds_cfg)
    monkeypatch.setenv("DEEPEMIA_WORKERS", "1")
    _run_cli_plain(monkeypatch, cfgdir, tmp_path)
    names = ("neighbours_results.csv", "measurements_results.csv", "R50_flip_results.csv")
    single = {nm: (split / nm).read_bytes() for nm in names}
    rows = list(csv.reader(io.StringIO(single["neighbours_results.csv"].decode(), newline="")))
    assert len(rows) > 20 and {r[13] for r in rows[1:]} == {f"em_{i}.tif" for i in range(5)}
    for nm in names:
        (split / nm).unlink()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = mp.Manager().dict()
    mp.spawn(_cli_rank_worker, args=(2, port, str(tmp_path), str(cfgdir), None, None, None, None, out, "images"), nprocs=2, join=True)
    assert dict(out) == {0: 0, 1: 0}
    for nm in names:
        assert (split / nm).read_bytes() == single[nm], nm
