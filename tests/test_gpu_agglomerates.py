"""``demia_mask_agglomerates`` / ``demia_crop_agglomerates`` -- the link graph between the masks of a frame, its components and the
moments that count a shared pixel once -- against the literal reference of ``tests/agglomerate_ref.py`` on the scenes of
``tests/agglomerate_cases.py`` and on seeded random scenes, integer for integer; then the matrix's shape, crops against planes,
position and order invariance, the shared border stage, the bounds of every output, both label paths, the ride in
``ContourSet.fetch`` and the CLI in every mask frame and over two ranks."""
import csv
import io

import numpy as np
import pytest

import agglomerate_cases as AC
import agglomerate_ref as AR
import neighbour_ref as NR

pytestmark = pytest.mark.gpu

CANARY = 0x5A5A5A5A
GUARD = 64                       # int32 words of canary on either side of every output
SCENES = AC.by_name()


@pytest.fixture(scope="module")
def ops(gpu_device):
    from deepemia_amd.maskset import MaskOps
    return MaskOps(gpu_device)


@pytest.fixture(scope="module")
def refs():
    """name -> links, degree, label, own of the reference, computed once and shared."""
    return {n: AR.everything(s.masks, s.group, s.l2) for n, s in SCENES.items()}


def _planes(ops, masks):
    ops.set_frame_width(masks.shape[2])
    return ops.from_dense(masks)


def _run_planes(ops, s, **kw):
    return ops.agglomerates(_planes(ops, s.masks), None, None, group=s.group, l2=s.l2, label_lds_cap=s.cap, **kw)


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


def _host(ag):
    return {"links": ag.links.cpu().numpy().view(np.uint32).tolist(), "degree": ag.degree.cpu().numpy().tolist(),
            "label": ag.label.cpu().numpy().tolist(), "own": ag.own.cpu().numpy().tolist()}


def _check_shape(got, M):
    """links is symmetric with a zero diagonal and zero pad bits; degree is its popcount."""
    lk = got["links"]
    assert len(lk) == M and all(len(r) == (M + 31) // 32 for r in lk)
    bit = [[(lk[a][b >> 5] >> (b & 31)) & 1 for b in range(32 * ((M + 31) // 32))] for a in range(M)]
    for a in range(M):
        assert not bit[a][a] and not any(bit[a][M:]), a
        assert all(bit[a][b] == bit[b][a] for b in range(M)), a
        assert got["degree"][a] == sum(bit[a]), a


# ------------------------------------------------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("name", list(SCENES))
def test_both_entries_equal_the_reference(ops, refs, name):
    s = SCENES[name]
    want = refs[name]
    got = _host(_run_planes(ops, s))
    for key in ("links", "degree", "label", "own"):
        assert got[key] == want[key], key
    _check_shape(got, s.masks.shape[0])
    gc = _host(_crops(ops, s.masks).agglomerates(group=s.group, l2=s.l2, label_lds_cap=s.cap))
    assert gc == want
    if s.group is None:
        assert sum(o[0] for o in got["own"]) == int(np.logical_or.reduce(s.masks, axis=0).sum())


def test_random_scenes_equal_the_reference(ops):
    for seed in AC.RANDOM_SEEDS:
        s = AC.random_scene(seed)
        want = AR.everything(s.masks, s.group, s.l2)
        got = _host(_run_planes(ops, s))
        assert got == want, seed
        _check_shape(got, s.masks.shape[0])
        gc = _host(_crops(ops, s.masks, grow=40 if seed % 2 else None, seed=seed).agglomerates(group=s.group, l2=s.l2))
        assert gc == want, seed
        if s.group is None:
            assert sum(o[0] for o in got["own"]) == int(np.logical_or.reduce(s.masks, axis=0).sum()), seed


def test_degree_at_touching_is_the_neighbour_stage_s_count(ops):
    for seed in (0, 4, 7, 13):
        masks = AC.random_scene(seed).masks
        planes = _planes(ops, masks)
        nb = ops.neighbours(planes, None, None, group=None, r2=-1)
        ag = ops.agglomerates(planes, None, None, group=None, l2=2)
        assert ag.degree.cpu().numpy().tolist() == nb.table.cpu().numpy()[:, 4].tolist(), seed
    s = SCENES["chain_cap_0"]
    planes = _planes(ops, s.masks)
    assert ops.agglomerates(planes, None, None).degree.cpu().numpy().tolist() == ops.neighbours(planes, None, None).table.cpu().numpy()[:, 4].tolist()


# ------------------------------------------------------------------------------------------------------- 2. crops against planes
@pytest.mark.parametrize("name", ["overlaps", "contained", "disc_in_hole", "corners_edges", "empty_among", "last_column", "long_border", "interleaved_l2_4"])
def test_crops_equal_planes_in_tight_and_grown_rooms(ops, name):
    import torch
    s = SCENES[name]
    ap = _run_planes(ops, s)
    for grow, seed in ((None, 0), (40, 1), (40, 2), (7, 3)):
        ac = _crops(ops, s.masks, grow=grow, seed=seed).agglomerates(group=s.group, l2=s.l2)
        for key in ("links", "degree", "label", "own", "sums", "nborder"):
            assert torch.equal(getattr(ac, key), getattr(ap, key)), (key, grow, seed)


def test_selected_subset_equals_the_reference_on_that_subset(ops):
    for seed in (5, 11, 24):
        s = AC.random_scene(seed)
        M = s.masks.shape[0]
        group = s.group if s.group is not None else np.zeros(M, dtype=np.int32)
        idx = np.random.default_rng(seed).permutation(M)[: max(2, M // 2)]
        sub = _crops(ops, s.masks, grow=12, seed=seed).select(idx)
        assert _host(sub.agglomerates(group=group[idx], l2=s.l2)) == AR.everything(s.masks[idx], group[idx], s.l2), seed


# ------------------------------------------------------------------------------------------------------- 3. invariance
def test_translation_by_33_17(ops):
    for seed in (1, 2, 3):
        s = AC.random_scene(seed)
        M, H, W = s.masks.shape
        a = np.zeros((M, H + 30, W + 45), dtype=bool)
        b = np.zeros_like(a)
        a[:, :H, :W] = s.masks
        b[:, 17:17 + H, 33:33 + W] = s.masks
        ga = _host(ops.agglomerates(_planes(ops, a), None, None, group=s.group, l2=s.l2))
        gb = _host(ops.agglomerates(_planes(ops, b), None, None, group=s.group, l2=s.l2))
        assert ga == AR.everything(s.masks, s.group, s.l2)
        assert (gb["links"], gb["degree"], gb["label"]) == (ga["links"], ga["degree"], ga["label"])
        dx, dy = 33, 17
        assert gb["own"] == [[n, sx + dx * n, sy + dy * n, sxx + 2 * dx * sx + dx * dx * n, syy + 2 * dy * sy + dy * dy * n,
                              sxy + dx * sy + dy * sx + dx * dy * n] for n, sx, sy, sxx, syy, sxy in ga["own"]]


def test_permutation_of_the_masks_permutes_the_partition(ops):
    def parts(label, back):
        out = {}
        for i, v in enumerate(label):
            if v >= 0:
                out.setdefault(v, set()).add(back[i])
        return sorted(map(sorted, out.values()))
    for name in ("chain_cap_0", "overlaps", "classes_same", "two_chains_l2_2"):
        s = SCENES[name]
        M = s.masks.shape[0]
        perm = np.random.default_rng(7).permutation(M)
        group = None if s.group is None else s.group[perm]
        g0 = _host(_run_planes(ops, s))
        g1 = _host(ops.agglomerates(_planes(ops, s.masks[perm]), None, None, group=group, l2=s.l2))
        assert g1 == AR.everything(s.masks[perm], group, s.l2), name                # labels are the smallest index of the NEW order
        assert parts(g1["label"], perm.tolist()) == parts(g0["label"], list(range(M))), name
        assert [g1["degree"][i] for i in range(M)] == [g0["degree"][p] for p in perm.tolist()], name


# ------------------------------------------------------------------------------------------------------- 4. the shared border stage
@pytest.mark.parametrize("frame", ["planes", "crops"])
def test_reusing_the_neighbour_stage_s_border_changes_nothing(ops, frame):
    import torch
    for seed in (3, 8, 21):
        s = AC.random_scene(seed)
        group = s.group if s.group is not None else np.zeros(len(s.masks), dtype=np.int32)
        if frame == "planes":
            planes = _planes(ops, s.masks)
            area = s.masks.reshape(len(s.masks), -1).sum(1)
            bbox = ops.upload(NR.tight_boxes(s.masks))
            alone_nb = ops.neighbours(planes, bbox, area, group=group, r2=30)
            alone = ops.agglomerates(planes, bbox, area, group=s.group, l2=s.l2)
            nb = ops.neighbours(planes, bbox, area, group=group, r2=30)
            ag = ops.agglomerates(planes, bbox, area, group=s.group, l2=s.l2, border=nb)
        else:
            cs = _crops(ops, s.masks, grow=9, seed=seed)
            alone_nb = cs.neighbours(group=group, r2=30)
            alone = cs.agglomerates(group=s.group, l2=s.l2)
            nb = cs.neighbours(group=group, r2=30)
            ag = cs.agglomerates(group=s.group, l2=s.l2, border=nb)
        assert ag.points is nb.points and ag.sums is nb.sums and ag.nborder is nb.nborder
        for key in ("links", "degree", "label", "own", "sums", "nborder"):
            assert torch.equal(getattr(ag, key), getattr(alone, key)), (key, seed)
        # ... and the neighbour stage's own outputs are what they are without the new stage behind it
        for key in ("table", "sums", "nborder"):
            assert torch.equal(getattr(nb, key), getattr(alone_nb, key)), (key, seed)
        pa, pb, off = nb.points.cpu().numpy(), alone_nb.points.cpu().numpy(), nb.point_off
        nbd = nb.nborder.cpu().numpy()
        for m in range(len(s.masks)):
            assert sorted(pa[off[m]:off[m] + nbd[m]].tolist()) == sorted(pb[off[m]:off[m] + nbd[m]].tolist())
        assert (nb.table.cpu().numpy().tolist(), nb.sums.cpu().numpy().tolist()) == (NR.table(s.masks, group, 30), NR.sums(s.masks))


# ------------------------------------------------------------------------------------------------------- 5. bounds
@pytest.mark.parametrize("name", ["corners_edges", "empty_among", "row_word_edges_33", "chain_cap_64", "long_border", "interleaved_l2_2", "many_lower"])
@pytest.mark.parametrize("frame", ["planes", "crops"])
def test_nothing_is_written_outside_the_outputs(ops, refs, name, frame):
    """Every output of the C entries carved out of one canary buffer: only points[0 .. point_off[M]), nborder, sums, links, degree,
    label and own change -- and of the points only each mask's first nborder."""
    import torch

    from deepemia_amd import _lib
    from deepemia_amd.maskset import neighbour_offsets
    s = SCENES[name]
    M, H, W = s.masks.shape
    wpl = (M + 31) // 32
    off = neighbour_offsets(s.masks.reshape(M, -1).sum(1))
    total = int(off[-1])
    even = lambda n: n + (n & 1)                                                  # (even, so the int64 tables stay aligned)
    sizes = [even(total), even(M), 2 * 3 * M, even(M * wpl), even(M), even(M), 2 * 6 * M]
    flat = torch.from_numpy(np.full(sum(sizes) + GUARD * (len(sizes) + 1), CANARY, dtype=np.uint32).view(np.int32)).to(ops.device)
    views, pos = [], GUARD
    for n in sizes:
        views.append(flat[pos:pos + n])
        pos += n + GUARD
    points, nborder, sums, links, degree, label, own = views
    off_d = ops.upload(off)
    group_d = None if s.group is None else ops.upload(s.group)
    planes = _planes(ops, s.masks)
    bbox = ops.upload(NR.tight_boxes(s.masks))
    tail = (_lib.ptr(off_d), _lib.ptr(points), _lib.ptr(nborder), _lib.ptr(sums), 0, _lib.ptr(links), _lib.ptr(degree), _lib.ptr(label),
            _lib.ptr(own), s.cap, ops._stream())
    if frame == "planes":
        st = ops.lib.demia_mask_agglomerates(_lib.ptr(planes), _lib.ptr(bbox), _lib.ptr(group_d), M, H, W, s.l2, *tail)
    else:
        cs = _crops(ops, s.masks, grow=9, seed=4)
        st = ops.lib.demia_crop_agglomerates(_lib.ptr(cs.payload), _lib.ptr(cs.room), _lib.ptr(cs.offsets), _lib.ptr(cs.bbox), _lib.ptr(group_d),
                                             M, H, W, s.l2, *tail)
    _lib.check(st, "agglomerates")
    host = flat.cpu().numpy().view(np.uint32)
    keep = np.ones(host.shape, dtype=bool)
    pos = GUARD
    for n, used in zip(sizes, [total, M, 6 * M, M * wpl, M, M, 12 * M]):
        keep[pos:pos + used] = False                                              # (the padding word of an odd size stays a canary too)
        pos += n + GUARD
    assert (host[keep] == CANARY).all()
    nb_h = nborder.cpu().numpy()[:M]
    pts = points.cpu().numpy().view(np.uint32)
    for m in range(M):
        assert (pts[off[m] + nb_h[m]: off[m + 1]] == CANARY).all(), m
    want = refs[name]
    assert links[:M * wpl].cpu().numpy().view(np.uint32).reshape(M, wpl).tolist() == want["links"]
    assert degree[:M].cpu().numpy().tolist() == want["degree"] and label[:M].cpu().numpy().tolist() == want["label"]
    assert own.view(torch.int64).view(M, 6).cpu().numpy().tolist() == want["own"]
    assert sums.view(torch.int64).view(M, 3).cpu().numpy().tolist() == NR.sums(s.masks)


def test_both_label_paths_agree(ops):
    import torch
    for name in ("chain_cap_0", "two_chains_l2_2", "two_chains_l2_4", "row_word_edges_65", "empty_among"):
        s = SCENES[name]
        planes = _planes(ops, s.masks)
        got = [ops.agglomerates(planes, None, None, group=s.group, l2=s.l2, label_lds_cap=cap).label for cap in (0, 64, 1, 1 << 20)]
        assert all(torch.equal(got[0], g) for g in got[1:]), name
        cs = _crops(ops, s.masks)
        assert torch.equal(cs.agglomerates(group=s.group, l2=s.l2, label_lds_cap=2).label, got[0]), name


def test_no_masks_and_bad_arguments(ops):
    import torch

    from deepemia_amd import _lib
    t = torch.full((64,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=ops.device)
    p = _lib.ptr(t)
    lib, st = ops.lib, ops._stream()
    assert lib.demia_mask_agglomerates(0, 0, 0, 0, 40, 70, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, st) == 0
    assert lib.demia_crop_agglomerates(0, 0, 0, 0, 0, 0, 40, 70, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, st) == 0
    assert lib.demia_mask_agglomerates(p, p, 0, 0, 40, 70, 2, p, p, p, p, 0, p, p, p, p, 0, st) == 0      # M = 0 touches nothing
    for H, W in ((0, 70), (40, 0), (32768, 70), (40, 32768)):
        assert lib.demia_mask_agglomerates(p, p, 0, 1, H, W, 2, p, p, p, p, 0, p, p, p, p, 0, st) != 0
    for M in (-1, 32769):
        assert lib.demia_mask_agglomerates(p, p, 0, M, 40, 70, 2, p, p, p, p, 0, p, p, p, p, 0, st) != 0
    for l2 in (1, 0, -1):
        assert lib.demia_mask_agglomerates(p, p, 0, 1, 40, 70, l2, p, p, p, p, 0, p, p, p, p, 0, st) != 0
    for hole in range(4):                                                        # a missing output
        outs = [p] * 4
        outs[hole] = 0
        assert lib.demia_mask_agglomerates(p, p, 0, 1, 40, 70, 2, p, p, p, p, 0, *outs, 0, st) != 0
    assert lib.demia_mask_agglomerates(p, p, 0, 1, 40, 70, 2, p, 0, p, p, 1, p, p, p, p, 0, st) != 0
    assert lib.demia_crop_agglomerates(p, 0, p, p, 0, 1, 40, 70, 2, p, p, p, p, 0, p, p, p, p, 0, st) != 0
    with pytest.raises(_lib.HipKernelError, match="32768"):
        _lib.check(lib.demia_mask_agglomerates(p, p, 0, 32769, 40, 70, 2, p, p, p, p, 0, p, p, p, p, 0, st), "demia_mask_agglomerates")
    with pytest.raises(_lib.HipKernelError, match="32767"):
        _lib.check(lib.demia_mask_agglomerates(p, p, 0, 1, 40, 32768, 2, p, p, p, p, 0, p, p, p, p, 0, st), "demia_mask_agglomerates")
    assert (t.cpu().numpy() == 0x5A5A5A5A5A5A5A5A).all()                        # no refused call and no M = 0 call wrote anything
    from deepemia_amd.cropset import CropMaskSet
    ag = ops.agglomerates(_planes(ops, np.zeros((0, 40, 70), dtype=bool)), None, None)
    assert tuple(ag.links.shape) == (0, 0) and tuple(ag.own.shape) == (0, 6) and tuple(ag.label.shape) == (0,)
    assert tuple(CropMaskSet.empty(ops, (40, 70)).agglomerates().own.shape) == (0, 6)


# ------------------------------------------------------------------------------------------------------- 6. the ride in the fetch
@pytest.mark.parametrize("frame", ["planes", "crops"])
def test_tables_ride_in_the_contour_fetch(ops, monkeypatch, frame):
    import torch

    from deepemia_amd.maskset import Agglomerates, Neighbours
    s = AC.random_scene(9)
    masks = s.masks[[k for k in range(len(s.masks)) if s.masks[k].any()]]
    group = np.arange(len(masks), dtype=np.int32) % 2
    planes = _planes(ops, masks)
    area = masks.reshape(len(masks), -1).sum(1)
    bbox = ops.upload(NR.tight_boxes(masks))
    if frame == "planes":
        cs = ops.trace(planes, max_contours=64, bbox=bbox, total_area=int(area.sum()))
        nb = ops.neighbours(planes, bbox, area, group=group, r2=30)
        ag = ops.agglomerates(planes, bbox, area, group=group, l2=5, border=nb)
    else:
        cset = _crops(ops, masks, grow=5)
        cs = cset.trace(max_contours=64, total_area=int(area.sum()))
        nb = cset.neighbours(area=area, group=group, r2=30)
        ag = cset.agglomerates(area=area, group=group, l2=5, border=nb)
    cs.launch_measure(1.0, slots=4)
    copies = [0]
    cpu = torch.Tensor.cpu

    def spy(self, *a, **k):
        copies[0] += 1
        return cpu(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "cpu", spy)
    got = cs.fetch(extra=[nb.table_i32, nb.sums_i32] + ag.ride, with_points=True)
    monkeypatch.undo()
    assert copies[0] == 1                                                        # the one copy of the fetch brought the tables too
    assert sum(int(t.numel()) * 4 for t in ag.ride) == 56 * len(masks)
    t, sm = Neighbours.from_i32(got[-5], got[-4])
    assert (t.tolist(), sm.tolist()) == (NR.table(masks, group, 30), NR.sums(masks))
    lab, deg, own = Agglomerates.from_i32(*got[-3:])
    want = AR.everything(masks, group, 5)
    assert (lab.tolist(), deg.tolist(), own.tolist()) == (want["label"], want["degree"], want["own"])


# ------------------------------------------------------------------------------------------------------- 7. CLI
GAP = 2.5                        # pixels (no scale bar): L2 = 6


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory, gpu_device):
    """``main.py --task inference`` on two small images, once per (mask frame, setting): the output files of every run, the
    pipeline's ``d2h_waits`` and the device-to-host copies it made."""
    import torch

    import main as cli
    from deepemia_amd.functions import inference as inf_mod
    from deepemia_amd.utils import config as C
    from test_gpu_cropset import DATASET, _set_frame, _write_tree

    tmp_path = tmp_path_factory.mktemp("agglomerates_cli")
    ds_cfg = {"inference_overrides": {"confidence_mode": "manual",
                                      "class_specific_settings": {"class_0": {"confidence_threshold": 0.3, "iou_threshold": 0.6},
                                                                  "class_1": {"confidence_threshold": 0.35, "iou_threshold": 0.5}},
                                      "tile_settings": {"tile_size": 200, "overlap_ratio": 0.125, "upscale_factor": 1.0, "edge_filter_enabled": True},
                                      "spatial_constraints": {"enabled": True, "containment_rules": {1: 0}, "containment_threshold": 0.5}}}
    on = {"agglomerate_statistics": True}
    runs = (("full", "off", {}), ("full", "on", on), ("crop", "on", on), ("crop_direct", "on", on),
            ("full", "both", dict(on, neighbour_statistics=True)), ("full", "nb", {"neighbour_statistics": True}),
            ("full", "gap", dict(on, agglomerate_gap=GAP, agglomerate_link="same_class")))
    names = ["measurements_results.csv", "R50_flip_results.csv", "neighbours_results.csv", "agglomerates_results.csv"]
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
    off = cli_runs["full", "off"]["files"]
    assert off["agglomerates_results.csv"] is None and off["neighbours_results.csv"] is None
    for key in (("full", "on"), ("crop", "on"), ("crop_direct", "on"), ("full", "both"), ("full", "gap")):
        on = cli_runs[key]["files"]
        assert on["agglomerates_results.csv"] is not None, key
        for nm in ("measurements_results.csv", "R50_flip_results.csv"):
            assert on[nm] == off[nm] and len(off[nm]) > 200, (key, nm)
    assert cli_runs["full", "on"]["files"]["neighbours_results.csv"] is None
    assert cli_runs["full", "nb"]["files"]["agglomerates_results.csv"] is None
    assert cli_runs["full", "both"]["files"]["neighbours_results.csv"] == cli_runs["full", "nb"]["files"]["neighbours_results.csv"] is not None


def test_cli_file_is_the_same_in_every_mask_frame_and_beside_the_neighbour_stage(cli_runs):
    ref = cli_runs["full", "on"]["files"]["agglomerates_results.csv"]
    for key in (("crop", "on"), ("crop_direct", "on"), ("full", "both")):
        assert cli_runs[key]["files"]["agglomerates_results.csv"] == ref, key


def test_cli_adds_no_wait_and_no_copy(cli_runs):
    off = cli_runs["full", "off"]
    for key in (("full", "on"), ("full", "both"), ("full", "gap")):
        on = cli_runs[key]
        assert on["d2h_waits"] == off["d2h_waits"] > 0, key
        assert on["copies"] == off["copies"] > 0, key                            # the tables came in a copy that was made anyway
    # (crop and crop_direct off are the neighbour tests' runs; the three frames agree on the stage's own cost: none)
    assert cli_runs["full", "nb"]["d2h_waits"] == off["d2h_waits"] and cli_runs["full", "nb"]["copies"] == off["copies"]


def _images(rle):
    return [r[0] for k, r in enumerate(rle) if k == 0 or rle[k - 1][0] != r[0]]


@pytest.mark.parametrize("label", ["on", "gap"])
def test_cli_values_equal_the_reference_on_the_masks_of_the_run(cli_runs, label):
    """The run's own ``R50_flip_results.csv`` decoded to dense masks, the reference on them, ``agglomerate_rows`` on the reference's
    integers, ``csv.writer``: the bytes of ``agglomerates_results.csv``; and the member ids partition each image's instance ids."""
    from deepemia_amd.functions.inference import AGGLOMERATE_CSV_HEADER, agglomerate_l2, agglomerate_rows
    from test_gpu_cropset import CLASSES
    from test_gpu_pipeline_e2e import _rle_decode
    files = cli_runs["full", label]["files"]
    got = list(csv.reader(io.StringIO(files["agglomerates_results.csv"].decode(), newline="")))
    assert got[0] == AGGLOMERATE_CSV_HEADER
    rle = list(csv.reader(io.StringIO(files["R50_flip_results.csv"].decode(), newline="")))[1:]
    nbr = list(csv.reader(io.StringIO(cli_runs["full", "nb"]["files"]["neighbours_results.csv"].decode(), newline="")))[1:]
    hw = {"em_0": (300, 417), "em_1": (260, 500)}
    l2 = agglomerate_l2(GAP if label == "gap" else None, 1.0)
    assert l2 == (6 if label == "gap" else 2)
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(AGGLOMERATE_CSV_HEADER)
    members_seen, multi = 0, 0
    for image in _images(rle):
        masks = np.stack([_rle_decode(r[1], *hw[image]) for r in rle if r[0] == image])
        name = image + ".tif"
        classes = [int(r[1]) for r in nbr if r[13] == name]                       # (the neighbour file has one row per instance: its class)
        assert len(classes) == len(masks) >= 3
        ref = AR.everything(masks, classes if label == "gap" else None, l2)
        for r in agglomerate_rows(name, classes, CLASSES, ref["label"], ref["degree"], ref["own"], [int(m.sum()) for m in masks], 1.0, "0"):
            w.writerow(r)
        mine = [r for r in got[1:] if r[16] == name]
        assert [r[0] for r in mine] == [f"{name}_A{k + 1}" for k in range(len(mine))]
        ids = [i for r in mine for i in r[2].split(" ")]
        assert sorted(ids) == sorted(f"{name}_{k + 1}" for k in range(len(masks))) and len(set(ids)) == len(ids)
        assert all(int(r[1]) == len(r[2].split(" ")) for r in mine)
        members_seen += len(ids)
        multi += sum(int(r[1]) > 1 for r in mine)
    assert members_seen == len(rle)
    assert buf.getvalue().encode() == files["agglomerates_results.csv"]
    if label == "on":
        assert multi > 0                                                         # (the scene has instances in contact)


def test_cli_two_ranks_sharded_by_image_write_the_single_process_file(tmp_path, monkeypatch, gpu_device):
    import socket

    import torch.multiprocessing as mp

    from test_gpu_pipeline_e2e import _cli_rank_worker, _run_cli_plain, _write_tree
    tile = {"tile_size": 256, "overlap_ratio": 0.125, "upscale_factor": 1.0, "edge_filter_enabled": True}
    ds_cfg = {"inference_overrides": {"confidence_mode": "manual", "agglomerate_statistics": True, "agglomerate_gap": 3, "neighbour_statistics": True,
                                      "class_specific_settings": {"class_0": {"confidence_threshold": 0.3, "iou_threshold": 0.6},
                                                                  "class_1": {"confidence_threshold": 0.35, "iou_threshold": 0.5}},
                                      "tile_settings": tile, "spatial_constraints": {"enabled": True, "containment_rules": {1: 0}, "containment_threshold": 0.5}}}
    cfgdir, split, sds, images = _write_tree(tmp_path, [50], 0.5, 6.0, 5, 512, ds_cfg)
    monkeypatch.setenv("DEEPEMIA_WORKERS", "1")
    _run_cli_plain(monkeypatch, cfgdir, tmp_path)
    names = ("agglomerates_results.csv", "neighbours_results.csv", "measurements_results.csv", "R50_flip_results.csv")
    single = {nm: (split / nm).read_bytes() for nm in names}
    rows = list(csv.reader(io.StringIO(single["agglomerates_results.csv"].decode(), newline="")))
    assert len(rows) > 10 and {r[16] for r in rows[1:]} == {f"em_{i}.tif" for i in range(5)}
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
