"""GPU tests of the error maps (``demia_mask_error_map`` / ``demia_crop_error_map``; ``--task evaluate --visualize``): both entries
against the dense reference (``error_map_ref``) on every scene of ``error_map_cases`` and on 32 random scenes, byte for byte and
integer for integer; crops in tight and in grown rooms against planes; a selected subset; permuted masks; the source image left as
it is and the outputs between canaries; refusals that launch nothing; the scorer with the flag off and on (launches and copies
counted); and ``evaluate_model`` end to end on a six-image synthetic dataset in predictor mode and in pipeline mode on planes and on
crops: every PNG against the reference painted from the masks the run wrote and the rasterised ground truth, the table against the
reference's counts, and the result files byte for byte with and without the flag."""
import csv
import hashlib
import json
import sys
from collections import OrderedDict
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parent))
import coco_ref as R  # noqa: E402
import error_map_cases as EC  # noqa: E402
import error_map_ref as ER  # noqa: E402
import outline_ref as OR  # noqa: E402

pytestmark = pytest.mark.gpu

SCENES = EC.scenes() + [EC.random_scene(k) for k in range(32)]
NAMES = [s.name for s in SCENES]
CANARY = 0xA5


@pytest.fixture(scope="module")
def ops():
    from deepemia_amd.maskset import MaskOps
    return MaskOps("cuda:0")


@pytest.fixture(scope="module")
def table():
    """The scenes and their reference pictures and counts, computed once and left as they are."""
    out = {}
    for s in SCENES:
        dst, counts = ER.error_map(s.det, s.d_state, s.gt, s.g_state, s.image, s.alpha, s.line, s.palette)
        dst.setflags(write=False)
        counts.setflags(write=False)
        out[s.name] = (s, dst, counts)
    return out


def _planes(ops, dense):
    M, H, W = dense.shape
    ops.set_frame_width(W)
    if M == 0:
        return torch.zeros((0, H, (W + 31) // 32), dtype=torch.int32, device=ops.device), torch.zeros((0, 4), dtype=torch.int32, device=ops.device)
    planes = ops.from_dense(dense)
    return planes, ops.area_bbox(planes)[1]


def _crop_set(ops, dense, grow_seed=None):
    """The masks as a crop set: rooms = the tight boxes, or grown by up to 40 pixels a side, differently per seed."""
    from deepemia_amd.cropset import CropMaskSet

    M, H, W = dense.shape
    if M == 0:
        return CropMaskSet.empty(ops, (H, W))
    planes, bbox = _planes(ops, dense)
    tight = CropMaskSet.from_planes(ops, planes, W)
    if grow_seed is None:
        return tight
    room = bbox.cpu().numpy().copy()
    g = np.random.RandomState(grow_seed).randint(0, 41, room.shape)
    ok = room[:, 0] >= 0
    room[:, 0], room[:, 1] = np.maximum(0, room[:, 0] - g[:, 0]), np.maximum(0, room[:, 1] - g[:, 1])
    room[:, 2], room[:, 3] = np.minimum(H - 1, room[:, 2] + g[:, 2]), np.minimum(W - 1, room[:, 3] + g[:, 3])
    room[~ok] = -1
    return tight.reroom(room)


def _host(dst, counts):
    assert dst.dtype == torch.uint8 and counts.dtype == torch.int64 and tuple(counts.shape) == (4,)
    return dst.cpu().numpy(), counts.cpu().numpy()


def _on_planes(ops, s, det=None, d_state=None, gt=None, g_state=None):
    det, gt = s.det if det is None else det, s.gt if gt is None else gt
    d, d_bbox = _planes(ops, det)
    g, g_bbox = _planes(ops, gt)
    image = torch.from_numpy(s.image).to(ops.device)
    got = ops.error_map(d, d_bbox, s.d_state if d_state is None else d_state, g, g_bbox, s.g_state if g_state is None else g_state, image,
                        s.alpha, s.line, s.palette, W=s.hw[1])
    assert np.array_equal(image.cpu().numpy(), s.image)                       # the source is only read
    return _host(*got)


def _on_crops(ops, s, seeds):
    d_set, g_set = _crop_set(ops, s.det, seeds[0]), _crop_set(ops, s.gt, seeds[1])
    image = torch.from_numpy(s.image).to(ops.device)
    got = d_set.error_map(g_set, s.d_state, s.g_state, image, s.alpha, s.line, s.palette)
    assert np.array_equal(image.cpu().numpy(), s.image)
    return _host(*got)


def _assert_equal(got, want, what):
    (dst, counts), (w_dst, w_counts) = got, want
    assert dst.shape == w_dst.shape and dst.dtype == np.uint8
    assert counts.tolist() == w_counts.tolist(), (what, counts.tolist(), w_counts.tolist())
    assert np.array_equal(dst, w_dst), (what, int((dst != w_dst).any(axis=2).sum()), np.argwhere((dst != w_dst).any(axis=2))[:5].tolist())


@pytest.mark.parametrize("name", NAMES)
def test_planes_equal_the_reference_byte_for_byte(ops, table, name):
    s, dst, counts = table[name]
    _assert_equal(_on_planes(ops, s), (dst, counts), name)


@pytest.mark.parametrize("name", NAMES)
def test_crops_in_tight_and_grown_rooms_equal_the_reference_and_the_planes(ops, table, name):
    s, dst, counts = table[name]
    for what, seeds in (("tight", (None, None)), ("grown", (1, 2))):
        _assert_equal(_on_crops(ops, s, seeds), (dst, counts), (name, what))
    _assert_equal(_on_crops(ops, s, (3, None)), _on_planes(ops, s), name)


@pytest.mark.parametrize("name", ["seams_w544", "interactions", "crowded_tile", "random_5"])
def test_a_selected_subset_equals_the_reference_on_that_subset(ops, name):
    s = next(c for c in SCENES if c.name == name)
    rng = np.random.RandomState(11)
    keep_d = np.sort(rng.choice(len(s.det), max(1, len(s.det) // 2), replace=False)) if len(s.det) else np.zeros(0, np.int64)
    keep_g = rng.permutation(len(s.gt))[:max(1, 2 * len(s.gt) // 3)] if len(s.gt) else np.zeros(0, np.int64)
    want = ER.error_map(s.det[keep_d], s.d_state[keep_d], s.gt[keep_g], s.g_state[keep_g], s.image, s.alpha, s.line, s.palette)
    d_set, g_set = _crop_set(ops, s.det, 4).select(keep_d), _crop_set(ops, s.gt, None).select(keep_g)
    image = torch.from_numpy(s.image).to(ops.device)
    got = _host(*d_set.error_map(g_set, s.d_state[keep_d], s.g_state[keep_g], image, s.alpha, s.line, s.palette))
    _assert_equal(got, want, name)
    _assert_equal(_on_planes(ops, s, s.det[keep_d], s.d_state[keep_d], s.gt[keep_g], s.g_state[keep_g]), want, name)


@pytest.mark.parametrize("name", ["seams_w518", "interactions", "crowded_tile", "thin_t3", "random_7"])
def test_permuting_the_masks_changes_nothing(ops, table, name):
    s, dst, counts = table[name]
    rng = np.random.RandomState(12)
    pd, pg = rng.permutation(len(s.det)), rng.permutation(len(s.gt))
    _assert_equal(_on_planes(ops, s, s.det[pd], s.d_state[pd], s.gt[pg], s.g_state[pg]), (dst, counts), name)


@pytest.mark.parametrize("frame", ["planes", "crops"])
@pytest.mark.parametrize("name", ["seams_w544", "seams_w543", "interactions_gray_other_palette", "no_masks"])
def test_outputs_sit_between_canaries_and_the_source_is_unchanged(ops, table, name, frame):
    """The entries themselves, on the caller's buffers: dst, the partial rows and the counts each between two runs of canary bytes.
    The frame whose rows start on 4-byte boundaries is painted once from an aligned source (planes) and once from a source one byte
    off (crops): the picture does not depend on how the bytes are moved."""
    from deepemia_amd import _lib

    s, w_dst, w_counts = table[name]
    H, W = s.hw
    C = s.image.shape[2]
    tiles = int(ops.lib.demia_error_map_tiles(H, W))
    pad = 64
    spad = pad + (1 if frame == "crops" and W % 4 == 0 else 0)
    sizes = [H * W * 3, tiles * 32, 32]
    offs = np.cumsum([pad] + [n + pad + (-n) % 8 for n in sizes])[:-1]            # 8-byte aligned starts
    buf = torch.full((int(offs[-1] + sizes[-1] + pad),), CANARY, dtype=torch.uint8, device=ops.device)
    assert buf.data_ptr() % 8 == 0
    src_buf = torch.full((spad + H * W * C + pad,), CANARY, dtype=torch.uint8, device=ops.device)
    src_buf[spad:spad + H * W * C] = torch.from_numpy(s.image.reshape(-1)).to(ops.device)
    pal = np.ascontiguousarray(ER.PALETTE if s.palette is None else s.palette, dtype=np.uint8)
    states = ops.upload(np.concatenate([s.d_state, s.g_state]).astype(np.int32)) if len(s.d_state) + len(s.g_state) else None
    D, G = len(s.det), len(s.gt)
    d_st, g_st = (_lib.ptr(states[:D]) if D else 0), (_lib.ptr(states[D:]) if G else 0)
    ptrs = [buf.data_ptr() + int(o) for o in offs]
    tail = (H, W, src_buf.data_ptr() + spad, C, ptrs[0], s.alpha, s.line, pal.ctypes.data, ptrs[1], ptrs[2], ops._stream())
    if frame == "planes":
        (d, d_bbox), (g, g_bbox) = _planes(ops, s.det), _planes(ops, s.gt)
        _lib.check(ops.lib.demia_mask_error_map(_lib.ptr(d), _lib.ptr(d_bbox), d_st, D, _lib.ptr(g), _lib.ptr(g_bbox), g_st, G, *tail), "planes")
    else:
        ds, gs = _crop_set(ops, s.det, 5), _crop_set(ops, s.gt, 6)
        _lib.check(ops.lib.demia_crop_error_map(_lib.ptr(ds.payload), _lib.ptr(ds.room), _lib.ptr(ds.offsets), _lib.ptr(ds.bbox), d_st, D,
                                                _lib.ptr(gs.payload), _lib.ptr(gs.room), _lib.ptr(gs.offsets), _lib.ptr(gs.bbox), g_st, G, *tail), "crops")
    host, src_host = buf.cpu().numpy(), src_buf.cpu().numpy()
    inside = np.zeros(len(host), dtype=bool)
    for o, n in zip(offs, sizes):
        inside[int(o):int(o) + n] = True
    assert (host[~inside] == CANARY).all()
    assert (src_host[:spad] == CANARY).all() and (src_host[-pad:] == CANARY).all() and np.array_equal(src_host[spad:-pad], s.image.reshape(-1))
    dst = host[int(offs[0]):int(offs[0]) + sizes[0]].reshape(H, W, 3)
    partial = host[int(offs[1]):int(offs[1]) + sizes[1]].copy().view(np.int64).reshape(tiles, 4)
    counts = host[int(offs[2]):int(offs[2]) + 32].copy().view(np.int64)
    _assert_equal((dst, counts), (w_dst, w_counts), (name, frame))
    assert partial.sum(axis=0).tolist() == w_counts.tolist() and (partial >= 0).all()          # every row written


class _Spy:
    """The library with its calls counted by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


@pytest.fixture
def spied(ops):
    lib = ops.lib
    ops.lib = _Spy(lib)
    yield ops
    ops.lib = lib


def test_bad_arguments_raise_and_launch_nothing(spied):
    ops = spied
    s = next(c for c in SCENES if c.name == "interactions")
    H, W = s.hw
    (d, d_bbox), (g, g_bbox) = _planes(ops, s.det), _planes(ops, s.gt)
    d_set, g_set = _crop_set(ops, s.det), _crop_set(ops, s.gt)
    image = torch.from_numpy(s.image).to(ops.device)
    del ops.lib.calls[:]

    def both(message, image=image, alpha=96, line=2, palette=None, d_state=s.d_state, g_state=s.g_state):
        with pytest.raises(ValueError, match=message):
            ops.error_map(d, d_bbox, d_state, g, g_bbox, g_state, image, alpha, line, palette, W=W)
        with pytest.raises(ValueError, match=message):
            d_set.error_map(g_set, d_state, g_state, image, alpha, line, palette)
    for alpha in (-1, 257, 96.0, "96", True, None):
        both("alpha must be an integer from 0 to 256", alpha=alpha)
    for line in (0, 5, 1.0, "2", False, None):
        both("line must be an integer from 1 to 4", line=line)
    for palette in (ER.PALETTE[:7], ER.PALETTE.reshape(-1), ER.PALETTE.astype(np.float32), ER.PALETTE.astype(np.int32) + 1, [[0, 0, 0]] * 8 + [[1, 1, 1]]):
        both("palette must be 8 BGR triples of bytes", palette=palette)
    for bad in (image[:-1], image[:, :-1], image[:, :, :2], image.to(torch.int32), image.cpu(), s.image):
        both("image must be a uint8 device tensor of the frame", image=bad)
    both("d_state must be", d_state=s.d_state[:-1])
    both("d_state must be", d_state=np.full(len(s.det), 3))
    both("g_state must be", g_state=np.full(len(s.gt), 4))
    both("g_state must be", g_state=np.full(len(s.gt), -1))
    # planes of another frame; a set over another frame
    with pytest.raises(ValueError, match="planes of"):
        ops.error_map(d, d_bbox, s.d_state, g[:, :-1].contiguous(), g_bbox, s.g_state, image, 96, 2, W=W)
    with pytest.raises(ValueError, match="pixels wide"):
        ops.error_map(d, d_bbox, s.d_state, g, g_bbox, s.g_state, image, 96, 2, W=W + 64)
    assert ops.lib.calls == []                              # not one call into the library so far
    other = _crop_set(ops, s.gt[:, :-1])
    del ops.lib.calls[:]
    with pytest.raises(ValueError, match="a set over"):
        d_set.error_map(other, s.d_state, s.g_state, image, 96, 2)
    assert ops.lib.calls == []
    # and a good call launches once
    ops.error_map(d, d_bbox, s.d_state, g, g_bbox, s.g_state, image, 96, 2, W=W)
    assert ops.lib.calls == ["demia_error_map_tiles", "demia_mask_error_map"]


# ---- the scorer ------------------------------------------------------------------------------------------------------------------
def _scoring_inputs(ops, H=300, W=518, n=40):
    """A record with ``n`` polygon annotations and one run-length crowd region, ``n`` detections near them (planes, host tables),
    and the image."""
    rng = np.random.RandomState(31)
    anns, centres = [], []
    for i in range(n):
        cx, cy = rng.uniform(30, W - 30), rng.uniform(30, H - 30)
        k = rng.randint(4, 10)
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        r = rng.uniform(6, 28, k)
        pts = np.round(np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1).reshape(-1), 2)
        anns.append({"segmentation": [[float(v) for v in pts]], "category_id": int(i % 2), "iscrowd": 0, "area": float(rng.uniform(50, 2000)),
                     "bbox": [float(cx - 28), float(cy - 28), float(cx + 28), float(cy + 28)], "bbox_mode": "XYXY_ABS"})
        centres.append((cx, cy))
    m = np.zeros((H, W), dtype=bool)
    m[100:150, 200:260] = rng.rand(50, 60) < .6
    anns.insert(7, {"segmentation": {"size": [H, W], "counts": [int(c) for c in R.encode(m)]}, "category_id": 0, "iscrowd": 1,
                    "area": float(m.sum()), "bbox": [200.0, 100.0, 260.0, 150.0], "bbox_mode": "XYXY_ABS"})
    rec = {"file_name": "some/where/synthetic.png", "image_id": 3, "height": H, "width": W, "annotations": anns}
    dense = np.zeros((n, H, W), dtype=bool)
    for i, (cx, cy) in enumerate(centres):
        dense[i] = EC._disc((H, W), cy + rng.randint(-3, 4), cx + rng.randint(-3, 4), rng.randint(8, 22)) & (rng.rand(H, W) < .95)
    planes, bbox = _planes(ops, dense)
    tabs = (dense.reshape(n, -1).sum(axis=1).astype(np.int64), bbox.cpu().numpy())
    scores = [float(v) for v in rng.uniform(.3, 1, n)]
    classes = [int(i % 2) for i in range(n)]
    image = np.random.RandomState(32).randint(0, 256, (H, W, 3)).astype(np.uint8)
    return rec, dense, planes, tabs, scores, classes, image


def test_scorer_flag_off_launches_and_copies_nothing_more_and_on_one_more_copy(spied, tmp_path):
    """One image through ``_score_pipeline_image`` on planes and on crops, without and with the error maps: the rows and the IoU
    tables are the same; off, no error-map entry is called and no copy is added; on, exactly one more ``Tensor.cpu()`` and one
    launch; the two frames write the same picture, and it is the reference's."""
    from deepemia_amd import cocoeval as CE
    from deepemia_amd.cropset import CropMaskSet
    from deepemia_amd.functions.evaluate_model import _new_tables, _score_pipeline_image

    ops = spied
    rec, dense, planes, tabs, scores, classes, image = _scoring_inputs(ops)
    H, W = image.shape[:2]
    image_dev = torch.from_numpy(image).to(ops.device)
    cset = CropMaskSet.from_planes(ops, planes, W, bbox=tabs[1], area=tabs[0])
    ids = {0: 0, 1: 1}
    copies, cpu = [0], torch.Tensor.cpu

    def spy_cpu(self, *a, **k):
        copies[0] += 1
        return cpu(self, *a, **k)
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", spy_cpu)
        for frame, masks in (("planes", planes), ("crops", cset)):
            for flag in (False, True):
                maps = CE.ErrorMaps(str(tmp_path / frame), 0.3, 96, None) if flag else None
                tables = _new_tables(None)
                copies[0] = 0
                del ops.lib.calls[:]
                rows = _score_pipeline_image(ops, rec, (H, W), masks, scores, classes, tabs, tables, ids, maps=maps,
                                             image=image_dev if flag else None)
                out[frame, flag] = dict(rows=rows, tables=tables, copies=copies[0], calls=[c for c in ops.lib.calls if "error_map" in c], maps=maps,
                                        wrote=(tmp_path / frame).exists())
    for frame in ("planes", "crops"):
        off, on = out[frame, False], out[frame, True]
        assert off["calls"] == [] and off["copies"] >= 1 and not off["wrote"] and on["wrote"]
        assert on["copies"] == off["copies"] + 1
        assert on["calls"] == ["demia_error_map_tiles", "demia_mask_error_map" if frame == "planes" else "demia_crop_error_map"]
        assert on["rows"] == off["rows"]
        for task in ("bbox", "segm"):
            for name in ("d_img", "d_cat", "d_score", "d_area", "d_row", "g_img", "g_cat", "g_area", "g_crowd", "g_col", "iou"):
                assert np.array_equal(on["tables"][task].cat(name), off["tables"][task].cat(name)), (frame, task, name)
    # the reference, from the dense detections and the rasterised ground truth
    anns = rec["annotations"]
    polys = [a["segmentation"] for a in anns if isinstance(a["segmentation"], list)]
    g_planes, _, _ = CE.rasterize_polygons(ops, polys, H, W)
    gt = list(ops.to_dense(g_planes, W))
    gt.insert(7, R.decode(anns[7]["segmentation"]["counts"], H, W))
    gt = np.stack(gt)
    crowd = [a["iscrowd"] for a in anns]
    iou = np.zeros((len(dense), len(gt)))
    for a, m in enumerate(dense):
        for b, g in enumerate(gt):
            inter = int(np.count_nonzero(m & g))
            if inter:
                iou[a, b] = inter / int(m.sum()) if crowd[b] else inter / (int(m.sum()) + int(g.sum()) - inter)
    pairs = OR.match(iou, scores, classes, [a["category_id"] for a in anns], crowd, 0.3)
    assert len(pairs) >= 10
    d_state, g_state = np.full(len(dense), 2), np.where(np.asarray(crowd) == 1, 3, 2)
    for d, g in pairs:
        d_state[d], g_state[g] = 1, 1
    want, counts = ER.error_map(dense, d_state, gt, g_state, image, 96, 1)
    assert counts[3] > 0                                                          # a detection reaches into the crowd region
    for frame in ("planes", "crops"):
        maps = out[frame, True]["maps"]
        path = tmp_path / frame / "evaluation_images" / "3_synthetic_evaluation.png"
        assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), want[:, :, ::-1]), frame
        assert maps.rows[0][:12] == [3, "synthetic.png", len(dense), len(gt) - 1, len(pairs), len(gt) - 1 - len(pairs), len(dense) - len(pairs), 1] + counts.tolist()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
DATASET = "synthpores"
CLASSES = ["pore", "throat"]
SIZE, IMAGES = 512, 6
FRAMES = OrderedDict([("predictor", ("predictor", "full", "planes")), ("planes", ("pipeline", "full", "planes")),
                      ("crops", ("pipeline", "crop_direct", "crops"))])
TODAY = ["coco_instances_results.json", "instances_predictions.pth", "metrics.csv"]


def _labels(rng, name, size):
    inst = []
    for j in range(6):
        cls = CLASSES[j % 2]
        if j == 5:
            inst.append({"type": "ellipse", "className": cls, "cx": float(rng.uniform(50, size - 50)), "cy": float(rng.uniform(50, size - 50)),
                         "rx": float(rng.uniform(5, 40)), "ry": float(rng.uniform(5, 40)), "angle": float(rng.uniform(0, 90))})
            continue
        cx, cy = rng.uniform(20, size - 20, 2)
        k = rng.randint(4, 10)
        ang = np.sort(rng.uniform(0, 2 * np.pi, k))
        r = rng.uniform(4, 60, k)
        pts = np.round(np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1).reshape(-1), 2)
        inst.append({"type": "polygon", "className": cls, "points": [float(v) for v in pts]})
    inst.append({"type": "polygon", "className": "unknown", "points": [1, 1, 5, 1, 5, 5]})
    return {"metadata": {"name": name, "height": size, "width": size}, "instances": inst}


def _dataset_cfg(mode, mask_frame, score_frame):
    inf = {"confidence_mode": "manual", "mask_frame": mask_frame,
           "class_specific_settings": {"class_0": {"confidence_threshold": 0.3, "iou_threshold": 0.6, "min_size": 25},
                                       "class_1": {"confidence_threshold": 0.35, "iou_threshold": 0.5, "min_size": 5}},
           "tile_settings": {"tile_size": 256, "overlap_ratio": 0.0, "upscale_factor": 1.0, "edge_filter_enabled": True},
           "ensemble_settings": {"enabled": False, "small_classes_only": False}}
    return {"inference_overrides": inf, "spatial_constraints": {"enabled": False},
            "evaluation": {"mode": mode, "max_dets": [1, 10, 1000], "score_frame": score_frame, "visualize_iou": 0.1}}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The six-image synthetic dataset (one R50 checkpoint; every image in the test split) and ``evaluate_model`` once per frame
    without and with ``visualize``: the output folder, what was returned and the device-to-host copies."""
    from deepemia_amd import synth
    from deepemia_amd.functions.evaluate_model import evaluate_model
    from deepemia_amd.utils import config as C

    root = tmp_path_factory.mktemp("errormaps")
    cfgdir, split = root / "cfg", root / "split_dir"
    (cfgdir / "datasets").mkdir(parents=True)
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
    (root / "imgs").mkdir()
    (root / "labels").mkdir()
    rng = np.random.RandomState(5)
    for i in range(IMAGES):
        name = f"em_{i}.png"
        Image.fromarray(synth.em_tile(60 + i, SIZE)[:, :, ::-1]).save(root / "imgs" / name, compress_level=1)
        lab = json.dumps(_labels(rng, name, SIZE))
        (root / "imgs" / f"em_{i}.json").write_text(lab)
        (root / "labels" / f"em_{i}.json").write_text(lab)
    (split / f"{DATASET}_split.json").write_text(json.dumps({"train": [], "test": sorted(f"em_{i}.json" for i in range(IMAGES))}))
    out = {"root": root}
    with pytest.MonkeyPatch.context() as mp:
        copies, cpu = [0], torch.Tensor.cpu

        def spy_cpu(self, *a, **k):
            copies[0] += 1
            return cpu(self, *a, **k)
        mp.setattr(torch.Tensor, "cpu", spy_cpu)
        mp.setenv("DEEPEMIA_CONFIG_DIR", str(cfgdir))
        mp.setenv("DEEPEMIA_OFFLINE", "1")
        mp.delenv("DEEPEMIA_EVAL_MODE", raising=False)
        mp.chdir(root)
        try:
            for frame, (mode, mask_frame, score_frame) in FRAMES.items():
                (cfgdir / "datasets" / f"{DATASET}.yaml").write_text(yaml.safe_dump(_dataset_cfg(mode, mask_frame, score_frame), sort_keys=False))
                for flag in (False, True):
                    C.reset_cache()
                    copies[0] = 0
                    where = root / f"{frame}_{'on' if flag else 'off'}"
                    res = evaluate_model(DATASET, str(where), visualize=flag, rcnn=50, mode=mode, threshold=0.3)
                    out[frame, flag] = dict(res=res, dir=where, copies=copies[0])
        finally:
            C.reset_cache()
    return out


def _sha(path):
    return hashlib.sha256(Path(path).read_bytes()).hexdigest()


def _png(path):
    return np.asarray(Image.open(path).convert("RGB"))


PICTURES = [f"{i}_em_{i}_evaluation.png" for i in range(IMAGES)]


@pytest.mark.parametrize("frame", list(FRAMES))
def test_flag_off_writes_todays_files_and_on_adds_the_maps_without_touching_them(runs, frame):
    off, on = runs[frame, False], runs[frame, True]
    assert sorted(p.name for p in off["dir"].iterdir()) == TODAY
    assert sorted(p.name for p in on["dir"].iterdir()) == sorted(TODAY + ["evaluation_images", "evaluation_images.csv"])
    assert sorted(p.name for p in (on["dir"] / "evaluation_images").iterdir()) == sorted(PICTURES + ["legend.png"])
    for f in ("coco_instances_results.json", "metrics.csv"):
        assert _sha(on["dir"] / f) == _sha(off["dir"] / f), f
    a = torch.load(off["dir"] / "instances_predictions.pth", weights_only=False)
    b = torch.load(on["dir"] / "instances_predictions.pth", weights_only=False)
    assert a == b and len(b) == IMAGES
    assert isinstance(on["res"], OrderedDict) and list(on["res"]) == list(off["res"]) == ["bbox", "segm"]
    for task in on["res"]:
        assert list(on["res"][task]) == list(off["res"][task])
        assert all(np.array_equal(on["res"][task][k], off["res"][task][k], equal_nan=True) for k in on["res"][task]), task
    assert on["copies"] == off["copies"] + IMAGES and off["copies"] > 0           # one more copy per image
    assert _png(on["dir"] / "evaluation_images" / "legend.png").shape[2] == 3


def test_planes_and_crops_write_the_same_pictures_and_table(runs):
    a, b = runs["planes", True]["dir"], runs["crops", True]["dir"]
    for f in ("coco_instances_results.json", "metrics.csv"):
        assert _sha(a / f) == _sha(b / f), f
    for name in PICTURES:
        assert np.array_equal(_png(a / "evaluation_images" / name), _png(b / "evaluation_images" / name)), name
    assert (a / "evaluation_images.csv").read_bytes() == (b / "evaluation_images.csv").read_bytes()


@pytest.fixture(scope="module")
def ground_truth(runs, ops):
    """Per image, in annotation order: the masks ``cocoeval.rasterize_polygons`` makes of the records' polygons, fetched to the host,
    and their categories."""
    from deepemia_amd import cocoeval as CE
    from deepemia_amd.data.datasets import read_dataset_info, register_datasets
    from deepemia_amd.functions.evaluate_model import _test_records
    from deepemia_amd.utils import config as C

    root = runs["root"]
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("DEEPEMIA_CONFIG_DIR", str(root / "cfg"))
        mp.setenv("DEEPEMIA_OFFLINE", "1")
        mp.chdir(root)
        C.reset_cache()
        try:
            info = read_dataset_info(root / "dataset_info.json")
            register_datasets(info, DATASET, dataset_format="json")
            recs, _, _ = _test_records(DATASET, "json", info, root / "split_dir")
        finally:
            C.reset_cache()
    out = {}
    for rec in recs:
        anns = rec["annotations"]
        planes, _, _ = CE.rasterize_polygons(ops, [a["segmentation"] for a in anns], SIZE, SIZE)
        out[rec["image_id"]] = (ops.to_dense(planes, SIZE), [int(a["category_id"]) for a in anns], rec["file_name"])
    assert sorted(out) == list(range(IMAGES)) and all(len(v[1]) >= 6 for v in out.values())
    return out


@pytest.mark.parametrize("frame", list(FRAMES))
def test_every_picture_and_row_equals_the_reference_on_the_runs_own_masks(runs, ground_truth, frame):
    from deepemia_amd import cocoeval as CE
    from deepemia_amd.functions.evaluate_model import read_image_bgr

    on = runs[frame, True]["dir"]
    found = json.loads((on / "coco_instances_results.json").read_text())
    rows = list(csv.reader(open(on / "evaluation_images.csv", newline="")))
    assert rows[0] == CE.ERROR_MAP_HEADER and len(rows) == 1 + IMAGES
    matched = filled = drawn = 0
    for i in range(IMAGES):
        gt, g_cat, file_name = ground_truth[i]
        mine = [r for r in found if r["image_id"] == i]
        det = np.stack([R.decode(R.from_string(r["segmentation"]["counts"]), SIZE, SIZE).astype(bool) for r in mine]) if mine \
            else np.zeros((0, SIZE, SIZE), dtype=bool)
        iou = np.zeros((len(det), len(gt)))
        for a, m in enumerate(det):
            for b, g in enumerate(gt):
                inter = int(np.count_nonzero(m & g))
                iou[a, b] = inter / (int(m.sum()) + int(g.sum()) - inter) if inter else 0.0
        pairs = OR.match(iou, [r["score"] for r in mine], [r["category_id"] for r in mine], g_cat, [0] * len(gt), 0.1)
        d_state, g_state = np.full(len(det), 2), np.full(len(gt), 2)
        for d, g in pairs:
            d_state[d], g_state[g] = 1, 1
        want, counts = ER.error_map(det, d_state, gt, g_state, read_image_bgr(file_name), 96, 1)
        assert np.array_equal(_png(on / "evaluation_images" / PICTURES[i]), want[:, :, ::-1]), (frame, i)
        agree, excess, missing, ignored = counts.tolist()
        ratio = [repr(n / d) if d else "" for n, d in ((agree, agree + excess), (agree, agree + missing), (2 * agree, 2 * agree + excess + missing))]
        assert rows[1 + i] == [str(v) for v in (i, f"em_{i}.png", len(det), len(gt), len(pairs), len(gt) - len(pairs), len(det) - len(pairs), 0,
                                               agree, excess, missing, ignored)] + ratio, (frame, i)
        matched += len(pairs)
        filled += agree
        drawn += len(det)
    print(f"{frame}: {drawn} detections, {matched} pairs, {filled} agreeing pixels over {IMAGES} images")
    assert drawn > 0
