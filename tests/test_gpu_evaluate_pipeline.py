"""GPU tests of the evaluate task's pipeline mode: the rasteriser, the cross matrix and the run-length kernels at 1 to 2048
masks of a 2048^2 frame against the CPU restatements; the instances the mode scores against the ones ``run_inference`` keeps
(one model, and the R50 + R101 ensemble); ``main.py --task evaluate`` end to end in pipeline mode (segm AP = the restated
COCOeval on the written results); the predictor mode unchanged by the new argument."""
import csv
import hashlib
import json
import math
import sys
import time
from collections import OrderedDict
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parent))
import coco_ref as R  # noqa: E402
import coco_ref_ext as X  # noqa: E402

pytestmark = pytest.mark.gpu

DATASET = "synthpores"
CLASSES = ["pore", "throat"]
FRAME = 2048


@pytest.fixture(scope="module")
def ops():
    from deepemia_amd.maskset import MaskOps
    return MaskOps("cuda:0")


# ---- kernels at pipeline-sized counts ---------------------------------------------------------------------------------------------
def _polygons(rng, n, size):
    """n small polygons spread over the frame: concave rings, the label files' 65-point ellipse rings, a mask of two polygons;
    the first ones sit on the right and bottom edges and in the corners (clipped by the frame)."""
    from deepemia_amd.data.datasets import ellipse_polygon

    spots = [(size - 3.0, size / 2), (size / 2, size - 2.0), (size - 4.0, size - 5.0), (20.0, 25.0)]
    masks = []
    for i in range(n):
        cx, cy = spots[i] if (i < len(spots) and n > 1) else rng.uniform(45, size - 45, 2)
        if i % 3 == 0:
            k = rng.randint(4, 10)
            ang = np.sort(rng.uniform(0, 2 * np.pi, k))
            r = rng.uniform(4, 40, k)
            masks.append([list(np.round(np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1).reshape(-1), 2))])
        elif i % 3 == 1:
            px, py = ellipse_polygon(cx, cy, rng.uniform(2, 30), rng.uniform(2, 30), rng.uniform(0, 180))
            masks.append([[c for x, y in zip(px, py) for c in (x + .5, y + .5)]])
        else:
            x0, y0 = int(cx) - 10, int(cy) - 12
            masks.append([[x0 + .5, y0 + .5, x0 + 18.5, y0 + .5, x0 + 18.5, y0 + 9.5, x0 + .5, y0 + 9.5],
                          [x0 + 12.5, y0 + 4.5, x0 + 30.5, y0 + 6.5, x0 + 14.5, y0 + 22.5]])
    return masks


def _blobs(rng, centres, size):
    """One random blob per centre (a noisy rectangle of up to 48 x 48 around it, every ninth empty, the second one with full
    columns at the bottom edge): (mask index, column-major position) of the set pixels, sorted per mask."""
    mi, pos = [], []
    for i, (cx, cy) in enumerate(centres):
        if i % 9 == 8:
            continue
        h, w = rng.randint(1, 48), rng.randint(1, 48)
        y0 = int(np.clip(cy - h // 2 + rng.randint(-6, 7), 0, size - h))
        x0 = int(np.clip(cx - w // 2 + rng.randint(-6, 7), 0, size - w))
        if i == 1:
            y0 = size - h
        sub = rng.rand(h, w) < (1.0 if i == 1 else .85)
        ys, xs = np.nonzero(sub)
        q = np.sort((xs + x0).astype(np.int64) * size + ys + y0)
        mi.append(np.full(len(q), i, dtype=np.int64))
        pos.append(q)
    if not pos:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(mi), np.concatenate(pos)


def _pack(ops, mi, pos, n, size):
    """Packed [n, size, size / 32] int32 on the device from (mask, column-major position) pixel lists."""
    x, y = pos // size, pos % size
    word = (mi * size + y) * (size // 32) + (x >> 5)
    uw, inv = np.unique(word, return_inverse=True)
    vals = np.zeros(len(uw), dtype=np.uint32)
    np.bitwise_or.at(vals, inv, (np.uint32(1) << (x & 31).astype(np.uint32)))
    packed = torch.zeros((n * size * (size // 32),), dtype=torch.int32, device=ops.device)
    packed[torch.from_numpy(uw).to(ops.device)] = torch.from_numpy(vals.view(np.int32)).to(ops.device)
    return packed.view(n, size, size // 32)


def _unpack(packed, size, chunk=128):
    """(mask, column-major position) of every set pixel of a packed device tensor, sorted by mask then position."""
    mi, pos = [], []
    for m0 in range(0, packed.shape[0], chunk):
        w = packed[m0:m0 + chunk].cpu().numpy().view(np.uint32)
        m, y, wx = np.nonzero(w)
        bits = (w[m, y, wx][:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1
        k, b = np.nonzero(bits)
        mi.append(m[k] + m0)
        pos.append((wx[k].astype(np.int64) * 32 + b) * size + y[k])
    mi, pos = np.concatenate(mi), np.concatenate(pos)
    order = np.lexsort((pos, mi))
    return mi[order], pos[order]


@pytest.mark.parametrize("n", [1, 100, 1000, 2048])
def test_kernels_at_pipeline_sized_counts(ops, n):
    """D = G = n on a 2048^2 frame: rasterised ground truth, |det & gt| of every pair and the detections' run lengths are
    bit-identical to ``coco_ref``'s rleFrPoly / encode and to the pixel-list intersection count."""
    from deepemia_amd import cocoeval as CE

    size = FRAME
    rng = np.random.RandomState(100 + n)
    t0 = time.perf_counter()
    polys = _polygons(rng, n, size)
    g_packed, g_area, g_bbox = CE.rasterize_polygons(ops, polys, size, size)
    # rasteriser: the union of every polygon's rleFrPoly runs
    want_pos = [np.unique(np.concatenate([X.runs_to_pixels(R.fr_poly(list(p), size, size)) for p in ps])) for ps in polys]
    want_mi = np.concatenate([np.full(len(q), i, dtype=np.int64) for i, q in enumerate(want_pos)])
    want_all = np.concatenate(want_pos)
    got_mi, got_pos = _unpack(g_packed, size)
    assert np.array_equal(got_mi, want_mi) and np.array_equal(got_pos, want_all)
    assert g_area.cpu().numpy().tolist() == [len(q) for q in want_pos]
    assert min(len(q) for q in want_pos[:4]) > 0
    bb = g_bbox.cpu().numpy()
    for i in range(0, n, max(1, n // 50)):
        q = want_pos[i]
        assert list(bb[i]) == [(q % size).min(), (q // size).min(), (q % size).max(), (q // size).max()]
    # detections: blobs near the ground truths, labels on both sides
    centres = [((q // size).mean(), (q % size).mean()) if len(q) else (size / 2, size / 2) for q in want_pos]
    d_mi, d_pos = _blobs(rng, centres, size)
    d_packed = _pack(ops, d_mi, d_pos, n, size)
    d_area, d_bbox = ops.area_bbox(d_packed)
    assert np.array_equal(d_area.cpu().numpy(), np.bincount(d_mi, minlength=n))
    dl, gl = rng.randint(0, 3, n), rng.randint(0, 3, n)
    want = X.cross_counts((d_mi, d_pos), (want_mi, want_all), n, n)
    got = CE.cross_matrix(ops, d_packed, d_bbox, dl, g_packed, g_bbox, gl, size).cpu().numpy()
    assert np.array_equal(got, want * (dl[:, None] == gl[None, :]))
    got = CE.cross_matrix(ops, d_packed, d_bbox, None, g_packed, g_bbox, None, size).cpu().numpy()
    assert np.array_equal(got, want)
    if n >= 100:
        assert np.count_nonzero(want) >= n // 2                     # the pairs do overlap
    # run lengths, strings and the box rule: both passes with a wait in between, and enqueued together into a sized room
    counts, off = CE.rle_counts(ops, d_packed, d_bbox, size)
    room = max(CE.rle_room(d_bbox.cpu().numpy()), int(off[-1]))      # (noisy blobs: more runs per column than the rule of thumb)
    n_t, c_t = CE.rle_counts_launch(ops, d_packed, d_bbox, size, room)
    runs = CE.rle_counts_finish(n_t.cpu().numpy(), c_t.cpu().numpy())
    assert runs is not None and np.array_equal(runs[0], counts) and np.array_equal(runs[1], off)
    tight = CE.rle_counts_finish(*[t.cpu().numpy() for t in CE.rle_counts_launch(ops, d_packed, d_bbox, size, max(1, int(off[-1]) - 1))])
    assert tight is None                                            # one count short: reported, nothing written out of its room
    strings = CE.rle_strings(counts, off)
    boxes = CE.rle_to_bbox(counts, off, size)
    split = np.searchsorted(d_mi, np.arange(n + 1))
    for i in range(n):
        want_runs = X.encode_pixels(d_pos[split[i]:split[i + 1]], size * size)
        assert counts[off[i]:off[i + 1]].tolist() == want_runs, i
        if i % max(1, n // 64) == 0 or i < 3:
            assert strings[i] == R.to_string(want_runs)
            assert list(boxes[i]) == X.to_bbox(want_runs, size, size)
    print(f"kernels at D = G = {n}: {time.perf_counter() - t0:.2f}s")


def test_sparse_helpers_equal_the_dense_restatements(ops):
    """The pixel-list helpers the 2048^2 cases rely on, against ``coco_ref``'s dense loops and the library's pack / unpack."""
    rng = np.random.RandomState(0)
    for _ in range(30):
        h, w = rng.randint(1, 9), rng.randint(1, 9)
        m = rng.rand(h, w) < rng.choice([0, .1, .5, .9, 1])
        r = R.encode(m)
        pos = np.flatnonzero(m.T.reshape(-1))
        assert X.encode_pixels(pos, h * w) == r and list(X.runs_to_pixels(r)) == list(pos)
    dense = rng.rand(5, 64, 64) < .2
    mi, rest = np.nonzero(dense.transpose(0, 2, 1).reshape(5, -1))
    packed = _pack(ops, mi, rest, 5, 64)
    assert (ops.to_dense(packed, 64) == dense).all()
    assert torch.equal(packed, ops.from_dense(dense))
    got = _unpack(packed, 64)
    assert np.array_equal(got[0], mi) and np.array_equal(got[1], rest)


# ---- the join and the CLI ------------------------------------------------------------------------------------------------------------
SIZE = 1024
N_IMAGES = 4
TILES = {"tile_size": 512, "overlap_ratio": 0.0, "upscale_factor": 1.0, "edge_filter_enabled": True}      # four tiles per image


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
    return {"metadata": {"name": name, "height": size, "width": size}, "instances": inst}


def _dataset_cfg(ensemble, evaluation=None):
    inf = {"confidence_mode": "manual",
           "class_specific_settings": {"class_0": {"confidence_threshold": 0.3, "iou_threshold": 0.6, "min_size": 25},
                                       "class_1": {"confidence_threshold": 0.35, "iou_threshold": 0.5, "min_size": 5}},
           "tile_settings": TILES, "ensemble_settings": {"enabled": bool(ensemble), "small_classes_only": False}}
    cfg = {"inference_overrides": inf, "spatial_constraints": {"enabled": False}}
    if evaluation is not None:
        cfg["evaluation"] = evaluation
    return cfg


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """Both models' checkpoints, four 1024^2 images with label files (all of them the test split) and the same images as the
    inference task's input folder."""
    from deepemia_amd import synth

    root = tmp_path_factory.mktemp("evalpipe")
    cfgdir = root / "cfg"
    (cfgdir / "datasets").mkdir(parents=True)
    split = root / "split_dir"
    base = {"bucket": None,
            "paths": {"split_dir": str(split), "category_json": str(root / "dataset_info.json"), "local_dataset_root": str(root)},
            "inference_settings": {"confidence_mode": "auto",
                                   "ensemble_settings": {"enabled": True, "small_classes_only": False, "weights": {"R50": 0.6, "R101": 0.4}},
                                   "spatial_constraints": {"default": {"enabled": False}}},
            "l4_performance_optimizations": {"enable_parallel_mask_processing": True}}
    (cfgdir / "config.yaml").write_text(yaml.safe_dump(base, sort_keys=False))
    (root / "dataset_info.json").write_text(json.dumps({DATASET: [str(root / "imgs"), str(root / "labels"), CLASSES]}))
    for d in (50, 101):
        sd = synth.random_d2_state_dict(d, len(CLASSES), seed=0, mask_bias=0.5, mask_gain=6.0)
        mdir = split / DATASET / f"rcnn_r{d}"
        mdir.mkdir(parents=True)
        synth.save_d2_checkpoint(str(mdir / f"model_final_r{d}.pth"), sd)
    inf = root / "DATASET" / "INFERENCE"
    for d in (root / "imgs", root / "labels", inf):
        d.mkdir(parents=True)
    rng = np.random.RandomState(5)
    for i in range(N_IMAGES):
        name = f"em_{i}.png"
        Image.fromarray(synth.em_tile(60 + i, SIZE)[:, :, ::-1]).save(root / "imgs" / name, compress_level=1)
        (inf / name).write_bytes((root / "imgs" / name).read_bytes())
        lab = json.dumps(_labels(rng, name, SIZE))
        (root / "imgs" / f"em_{i}.json").write_text(lab)
        (root / "labels" / f"em_{i}.json").write_text(lab)
    return root, cfgdir, split


def _configure(monkeypatch, tree, ds_cfg, test_names):
    from deepemia_amd.utils import config as C

    root, cfgdir, split = tree
    (cfgdir / "datasets" / f"{DATASET}.yaml").write_text(yaml.safe_dump(ds_cfg, sort_keys=False))
    split.mkdir(exist_ok=True)
    (split / f"{DATASET}_split.json").write_text(json.dumps({"train": [], "test": [n.replace(".png", ".json") for n in test_names]}))
    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(cfgdir))
    monkeypatch.setenv("DEEPEMIA_OFFLINE", "1")
    monkeypatch.delenv("DEEPEMIA_EVAL_MODE", raising=False)
    monkeypatch.chdir(root)
    C.reset_cache()


@pytest.mark.parametrize("rcnn,ensemble", [(50, False), ("combo", True)])
def test_pipeline_mode_scores_the_instances_run_inference_keeps(tree, monkeypatch, rcnn, ensemble):
    """Image by image: packed masks (``torch.equal``), scores and classes of the evaluate task's pipeline mode = those of
    ``run_inference`` with DEEPEMIA_KEEP_MASKS=1, in the same order.  (50, ensemble off): with both checkpoints on disk
    ``run_inference`` loads both and uses the first, R50, for every class -- what ``--rcnn 50`` evaluates alone.)"""
    import os

    from deepemia_amd.data.datasets import MetadataCatalog, read_dataset_info, register_datasets
    from deepemia_amd.functions.evaluate_model import PipelineRunner
    from deepemia_amd.functions.inference import run_inference
    from deepemia_amd.utils import config as C

    root, cfgdir, split = tree
    names = [f for f in os.listdir(root / "DATASET" / "INFERENCE")]          # run_inference's own order
    assert len(names) == N_IMAGES
    _configure(monkeypatch, tree, _dataset_cfg(ensemble), names)
    monkeypatch.setenv("DEEPEMIA_KEEP_MASKS", "1")
    try:
        kept = run_inference(DATASET, str(root / f"out_{rcnn}"), visualize=False, threshold=0.3)
        register_datasets(read_dataset_info(root / "dataset_info.json"), DATASET, dataset_format="json")
        runner = PipelineRunner(DATASET, MetadataCatalog.get(f"{DATASET}_train"), str(split), rcnn, 0.3)
        assert len(runner.pipe.predictors) == (2 if rcnn == "combo" else 1)
        total = 0
        for name, (path, hw, packed, scores, classes, tabs) in zip(names, runner.instances([str(root / "imgs" / n) for n in names])):
            want = kept[name]
            assert hw == (SIZE, SIZE) == tuple(want["hw"]) and path.endswith(name)
            assert want["masks"] is not None and want["masks"].shape[0] > 0, name
            assert torch.equal(packed, want["masks"]), name
            assert [float(s) for s in scores] == [float(s) for s in want["scores"]] and [type(s) for s in scores] == [type(s) for s in want["scores"]]
            assert [int(c) for c in classes] == [int(c) for c in want["classes"]]
            assert np.array_equal(tabs[0], want["area"]) and np.array_equal(tabs[1], want["bbox"])
            total += int(packed.shape[0])
        assert total >= N_IMAGES
        if ensemble:
            assert len(runner.st.models_needed(2, set(), len(CLASSES))) == 2
    finally:
        C.reset_cache()


def _metrics(split):
    rows = list(csv.reader(open(split / "metrics.csv")))
    assert rows[0] == ["metric", "value"] and [r[0] for r in rows[1:]] == ["bbox", "segm"]
    return {r[0]: eval(r[1], {"nan": float("nan")}) for r in rows[1:]}


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert (math.isnan(a[k]) and math.isnan(b[k])) or abs(a[k] - b[k]) <= 1e-12, (k, a[k], b[k])


def _sha(path):
    return hashlib.sha256(Path(path).read_bytes()).hexdigest()


def test_evaluate_cli_in_pipeline_mode_end_to_end(tree, monkeypatch, caplog):
    """``--task evaluate --rcnn combo`` with ``evaluation: {mode: pipeline}`` in the dataset's file: exit code 0, the three
    files, ``OrderedDict(bbox, segm)``; both tasks' metrics = ``coco_ref``'s COCOeval on the written detections (to 1e-12, as
    the predictor mode's CLI test)."""
    import main as cli
    from deepemia_amd.data.datasets import ellipse_polygon
    from deepemia_amd.functions.evaluate_model import evaluate_model
    from deepemia_amd.utils import config as C

    root, cfgdir, split = tree
    names = sorted(f"em_{i}.png" for i in range(N_IMAGES))
    _configure(monkeypatch, tree, _dataset_cfg(True, {"mode": "pipeline", "max_dets": [1, 10, 1000]}), names)
    for f in ("metrics.csv", "coco_instances_results.json", "instances_predictions.pth"):
        (split / f).unlink(missing_ok=True)
    try:
        t0 = time.perf_counter()
        assert cli.main(["--task", "evaluate", "--dataset_name", DATASET, "--rcnn", "combo", "--threshold", "0.3", "--no-gpu-check"]) == 0
        print(f"pipeline-mode CLI: {time.perf_counter() - t0:.2f}s")
        for f in ("metrics.csv", "coco_instances_results.json", "instances_predictions.pth"):
            assert (split / f).exists(), f
        res = json.loads((split / "coco_instances_results.json").read_text())
        assert sorted({r["image_id"] for r in res}) == list(range(N_IMAGES)) and len(res) >= N_IMAGES
        assert list(res[0]) == ["image_id", "category_id", "bbox", "score", "segmentation"]
        preds = torch.load(split / "instances_predictions.pth", weights_only=False)
        assert [p["image_id"] for p in preds] == list(range(N_IMAGES)) and sum(len(p["instances"]) for p in preds) == len(res)
        for r in res[:: max(1, len(res) // 40)]:                 # the box is toBbox of the mask's run lengths
            assert r["segmentation"]["size"] == [SIZE, SIZE]
            assert r["bbox"] == X.to_bbox(R.from_string(r["segmentation"]["counts"]), SIZE, SIZE)
        images, gts = R.gt_from_label_files(str(root / "labels"), [n.replace(".png", ".json") for n in names], CLASSES, ellipse_polygon)
        got = _metrics(split)
        for task in ("bbox", "segm"):
            stats, prec = X.coco_eval(images, gts, res, [0, 1], task, [1, 10, 1000])
            _same(got[task], R.derive(stats, prec, CLASSES))
        # the function itself: one model alone, the mode as an argument; returns Detectron2's OrderedDict
        C.reset_cache()
        out = evaluate_model(DATASET, str(root / "direct"), rcnn=50, mode="pipeline", threshold=0.3)
        assert isinstance(out, OrderedDict) and list(out) == ["bbox", "segm"]
        assert list(out["segm"])[:6] == ["AP", "AP50", "AP75", "APs", "APm", "APl"]
        _same(out["segm"], _metrics(root / "direct")["segm"])
    finally:
        C.reset_cache()


def test_predictor_mode_is_unchanged_by_the_mode_argument(tree, monkeypatch):
    """No key set: the CLI runs the predictor mode and refuses ``combo``; its files are byte-identical to
    ``evaluate_model(..., mode="predictor")`` called explicitly (the untouched predictor-mode tests pin the content)."""
    import main as cli
    from deepemia_amd.functions.evaluate_model import evaluate_model
    from deepemia_amd.utils import config as C

    root, cfgdir, split = tree
    names = sorted(f"em_{i}.png" for i in range(N_IMAGES))
    _configure(monkeypatch, tree, _dataset_cfg(True), names)
    try:
        assert cli.main(["--task", "evaluate", "--dataset_name", DATASET, "--rcnn", "combo", "--no-gpu-check"]) == 2
        t0 = time.perf_counter()
        assert cli.main(["--task", "evaluate", "--dataset_name", DATASET, "--rcnn", "50", "--no-gpu-check"]) == 0
        print(f"predictor-mode CLI: {time.perf_counter() - t0:.2f}s")
        C.reset_cache()
        out = evaluate_model(DATASET, str(root / "explicit"), rcnn=50, mode="predictor")
        assert isinstance(out, OrderedDict)
        for f in ("metrics.csv", "coco_instances_results.json"):
            assert _sha(split / f) == _sha(root / "explicit" / f), f
    finally:
        C.reset_cache()
