"""GPU tests of the outline-agreement report of ``--task evaluate`` (``evaluation.outline_agreement``): ``evaluate_model`` on the
boundary suite's scored tree in predictor mode and in pipeline mode on planes and on crops, with the switch off and on.  Off:
exactly today's three files.  On: the same three, byte for byte or value for value, and the two new ones; the rows of
``outline_agreement.csv`` equal the dense reference applied to the masks the run wrote and to ``coco_ref``'s rasterised ground
truth, value for value; one more device-to-host copy per image with a pair and no more pipeline waits.  One image through both
pipeline scorers: the same rows, and no full-frame tensor on crops.  The cost of the stage is printed, not asserted."""
import csv
import gc
import json
import sys
import time
from collections import OrderedDict
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import coco_ref as R  # noqa: E402
import outline_ref as OR  # noqa: E402
from test_gpu_boundary_eval import scored_tree  # noqa: E402,F401
from test_gpu_eval_crops import E2E_IMAGES, E2E_SIZE, _e2e_cfg, _scoring_inputs, small_tree  # noqa: E402,F401
from test_gpu_evaluate_pipeline import CLASSES, DATASET, _configure, _sha  # noqa: E402

pytestmark = pytest.mark.gpu

FRAMES = {"predictor": ("predictor", "full", "planes"), "planes": ("pipeline", "full", "planes"), "crops": ("pipeline", "crop_direct", "crops")}
TODAY = ["coco_instances_results.json", "instances_predictions.pth", "metrics.csv"]
NEW = ["outline_agreement.csv", "outline_summary.csv"]
IOU, TOLERANCE = 0.5, 2
ONE_IOU = 0.2                # the one-image test's threshold: its random boxes rarely reach 0.5 against their polygons


@pytest.fixture(scope="module")
def ops():
    from deepemia_amd.maskset import MaskOps
    return MaskOps("cuda:0")


@pytest.fixture(scope="module")
def runs(scored_tree):  # noqa: F811
    """``evaluate_model`` once per (frame, switch): what it returned, its output folder, the device-to-host copies it made and, in
    pipeline mode, the pipeline's own wait counter."""
    from deepemia_amd.functions import inference as inf_mod
    from deepemia_amd.functions.evaluate_model import evaluate_model
    from deepemia_amd.utils import config as C

    root, cfgdir, split = scored_tree
    names = sorted(f"em_{i}.png" for i in range(E2E_IMAGES))
    out = {}
    with pytest.MonkeyPatch.context() as mp:
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
        try:
            for frame, (mode, mask_frame, score_frame) in FRAMES.items():
                for switch in ("off", "on"):
                    cfg = _e2e_cfg(mask_frame, score_frame)
                    if switch == "on":
                        cfg["evaluation"]["outline_agreement"] = True
                    _configure(mp, scored_tree, cfg, names)
                    del pipes[:]
                    copies[0] = 0
                    where = root / f"outline_{frame}_{switch}"
                    res = evaluate_model(DATASET, str(where), rcnn=50, mode=mode, threshold=0.3)
                    out[frame, switch] = dict(res=res, dir=where, copies=copies[0], waits=pipes[-1].d2h_waits if pipes else None)
        finally:
            C.reset_cache()
    return out


_GT = {}


def _ground_truth(tree):
    """``coco_ref``'s rasterised ground truth of the tree's label files, per image in annotation order: (mask, category)."""
    from deepemia_amd.data.datasets import ellipse_polygon

    root = tree[0]
    if str(root) not in _GT:
        names = sorted(f"em_{i}.png" for i in range(E2E_IMAGES))
        images, gts = R.gt_from_label_files(str(root / "labels"), [n.replace(".png", ".json") for n in names], CLASSES, ellipse_polygon)
        hw = {im["id"]: (im["height"], im["width"]) for im in images}
        _GT[str(root)] = {i: [(R.poly_mask(g["segmentation"], *hw[i]), g["category_id"]) for g in gts if g["image_id"] == i] for i in hw}
    return _GT[str(root)]


def _reference_rows(tree, out_dir):
    """The rows the report must hold for the detections written to ``out_dir``: masks decoded on the CPU, IoU from pixel counts,
    the matching rule by brute force, the dense reference's records, the f64 formulas on its integers."""
    found = json.loads((Path(out_dir) / "coco_instances_results.json").read_text())
    rows, counts = [], {}
    for i, gt in sorted(_ground_truth(tree).items()):
        mine = [r for r in found if r["image_id"] == i]
        det = [R.decode(R.from_string(r["segmentation"]["counts"]), E2E_SIZE, E2E_SIZE).astype(bool) for r in mine]
        d_px, g_px = [int(m.sum()) for m in det], [int(m.sum()) for m, _ in gt]
        iou = np.zeros((len(det), len(gt)))
        for a, m in enumerate(det):
            for b, (g, _) in enumerate(gt):
                inter = int(np.count_nonzero(m & g))
                iou[a, b] = inter / (d_px[a] + g_px[b] - inter) if inter else 0.0
        d_cat, g_cat = [r["category_id"] for r in mine], [c for _, c in gt]
        pairs = OR.match(iou, [r["score"] for r in mine], d_cat, g_cat, [0] * len(gt), IOU)
        for c in g_cat:
            counts.setdefault(c, [0, 0, 0])[0] += 1
        for c in d_cat:
            counts.setdefault(c, [0, 0, 0])[1] += 1
        for d, g in pairs:
            counts[d_cat[d]][2] += 1
            dg, gd = OR.directed(det[d], gt[g][0]), OR.directed(gt[g][0], det[d])
            v = OR.values(dg, gd, d_px[d], g_px[g], TOLERANCE)
            rows.append([i, f"em_{i}.png", d_cat[d], CLASSES[d_cat[d]], d, g, mine[d]["score"], iou[d, g], d_px[d], g_px[g], dg["n"], gd["n"],
                         v["assd"], v["rms"], v["hausdorff"], v["hd95"], v["nsd"], v["diameter_error"], v["area_error"]])
    return rows, counts


def _csv(path):
    rows = list(csv.reader(open(path, newline="")))
    return rows[0], rows[1:]


@pytest.mark.parametrize("frame", list(FRAMES))
def test_switch_off_writes_todays_files_and_on_adds_two_without_touching_them(runs, frame):
    off, on = runs[frame, "off"], runs[frame, "on"]
    assert sorted(p.name for p in off["dir"].iterdir()) == TODAY
    assert sorted(p.name for p in on["dir"].iterdir()) == sorted(TODAY + NEW)
    for f in ("coco_instances_results.json", "metrics.csv"):
        assert _sha(on["dir"] / f) == _sha(off["dir"] / f), f
    a = torch.load(off["dir"] / "instances_predictions.pth", weights_only=False)
    b = torch.load(on["dir"] / "instances_predictions.pth", weights_only=False)
    assert a == b and len(b) == E2E_IMAGES
    # the returned dict: the same tasks, the same values, bit for bit
    assert isinstance(on["res"], OrderedDict) and list(on["res"]) == list(off["res"]) == ["bbox", "segm"]
    for task in on["res"]:
        assert list(on["res"][task]) == list(off["res"][task])
        assert all(np.array_equal(on["res"][task][k], off["res"][task][k], equal_nan=True) for k in on["res"][task]), task
    assert on["res"]["segm"]["AP"] > 0


@pytest.mark.parametrize("frame", list(FRAMES))
def test_rows_equal_the_reference_value_for_value(runs, scored_tree, frame):  # noqa: F811
    from deepemia_amd import cocoeval as CE

    on = runs[frame, "on"]
    want, counts = _reference_rows(scored_tree, on["dir"])
    head, got = _csv(on["dir"] / "outline_agreement.csv")
    assert head == CE.OUTLINE_ROW_HEADER
    assert len(got) == len(want) and {int(r[0]) for r in got} == set(range(E2E_IMAGES))          # at least one pair per image
    for g, w in zip(got, want):
        parsed = [int(g[0]), g[1], int(g[2]), g[3], int(g[4]), int(g[5])] + [float(v) for v in g[6:8]] + [int(v) for v in g[8:12]] + \
                 [float(v) for v in g[12:]]
        assert parsed == w, (frame, parsed, w)
    assert [(r[0], r[4]) for r in want] == sorted((r[0], r[4]) for r in want)                    # image order, then detection order
    assert any(r[12] > 0 for r in want) and any(r[17] != 0 for r in want)                        # the outlines are near, not equal
    # the summary: the counts of the reference, the pooled statistics of the rows
    head, summ = _csv(on["dir"] / "outline_summary.csv")
    assert head == CE.OUTLINE_SUMMARY_HEADER and [r[0] for r in summ] == CLASSES + ["all"]
    for r, cid in zip(summ, [0, 1, None]):
        cnt = [sum(v[k] for c, v in counts.items() if cid is None or c == cid) for k in range(3)]
        assert [int(v) for v in r[1:6]] == [cnt[0], cnt[1], cnt[2], cnt[0] - cnt[2], cnt[1] - cnt[2]]
        mine = [w for w in want if cid is None or w[2] == cid]
        if not mine:
            assert r[6:] == [""] * 7
            continue
        col = {k: np.asarray([w[12 + i] for w in mine]) for i, k in enumerate(CE.OUTLINE_VALUES)}
        stats = [col["assd"].mean(), np.median(col["assd"]), col["hd95"].mean(), col["hausdorff"].max(), col["nsd"].mean(),
                 col["diameter_error"].mean(), np.abs(col["area_error"]).mean()]
        assert [float(v) for v in r[6:]] == pytest.approx([float(s) for s in stats], rel=1e-14, abs=0)
    print(f"{frame}: all = {dict(zip(head, summ[-1]))}")


def test_the_three_frames_report_the_same_pairs_where_they_score_the_same_masks(runs):
    # planes and crops score the same pipeline: the same report, byte for byte
    for f in NEW:
        assert _sha(runs["planes", "on"]["dir"] / f) == _sha(runs["crops", "on"]["dir"] / f), f


@pytest.mark.parametrize("frame", list(FRAMES))
def test_one_more_copy_per_image_with_a_pair_and_no_more_waits(runs, frame):
    off, on = runs[frame, "off"], runs[frame, "on"]
    _, rows = _csv(on["dir"] / "outline_agreement.csv")
    with_pair = len({r[0] for r in rows})
    assert with_pair == E2E_IMAGES
    assert on["copies"] == off["copies"] + with_pair and off["copies"] > 0
    assert on["waits"] == off["waits"]
    if frame != "predictor":
        assert off["waits"] is not None


def test_one_image_through_both_scorers_same_rows_and_no_plane_on_crops(ops):
    """300 detections against 303 annotations (three of them run-length crowd regions) at 1024^2: the crop scorer with the switch
    on reports the rows of the plane scorer, makes exactly one more copy than with the switch off, leaves the IoU tables as they
    are, and its peak stays below a quarter of the planes the plane scorer holds -- no ``[*, H, W/32]`` tensor exists there.  The
    scoring time per image, off and on alternating in one process, is printed for both frames."""
    from deepemia_amd import cocoeval as CE
    from deepemia_amd.cropset import CropMaskSet
    from deepemia_amd.functions.evaluate_model import _new_tables, _score_pipeline_image

    size, n = 1024, 300
    rec, planes, tabs, scores, classes = _scoring_inputs(ops, size, n)
    ids = {0: 0, 1: 1}

    def score(masks, report, tables=None):
        return _score_pipeline_image(ops, rec, (size, size), masks, scores, classes, tabs, tables or _new_tables(None), ids, report=report)
    r_planes, t_planes, t_off = CE.OutlineReport(ONE_IOU, TOLERANCE), _new_tables(None), _new_tables(None)
    rows_planes = score(planes, r_planes, t_planes)
    rows_off = score(planes, None, t_off)
    assert rows_planes == rows_off and len(r_planes.rows) >= 60
    cset = CropMaskSet.from_planes(ops, planes, size, bbox=tabs[1], area=tabs[0])

    def timed(masks, on):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        score(masks, CE.OutlineReport(ONE_IOU, TOLERANCE) if on else None)
        return 1e3 * (time.perf_counter() - t0)
    for frame, masks in (("planes", planes), ("crops", cset)):
        timed(masks, True)                                                                     # (warm)
        t = {False: [], True: []}
        for _ in range(5):
            for on in (False, True):
                t[on].append(timed(masks, on))
        print(f"scoring on {frame}, {n} detections x {n + 3} annotations at {size}^2, {len(r_planes.rows)} pairs: "
              f"off {np.median(t[False]):.2f} ms/image, on {np.median(t[True]):.2f} ms/image (medians of 5, alternating)")
    del planes
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    copies, cpu = [0], torch.Tensor.cpu

    def spy(self, *a, **k):
        copies[0] += 1
        return cpu(self, *a, **k)
    r_crops, t_crops = CE.OutlineReport(ONE_IOU, TOLERANCE), _new_tables(None)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", spy)
        rows_crops = score(cset, r_crops, t_crops)
        copies_on, copies[0] = copies[0], 0
        score(cset, None)
        copies_off = copies[0]
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    plane_bytes = (n + n) * size * (size // 32) * 4
    print(f"crop scoring with the outline report, {n} x {n + 3} masks at {size}^2: peak {peak / 2**20:.2f} MiB, planes {plane_bytes / 2**20:.1f} MiB")
    assert peak < plane_bytes / 4
    assert copies_on == copies_off + 1 and copies_off >= 1
    assert rows_crops == rows_planes
    assert r_crops.rows == r_planes.rows and r_crops.counts == r_planes.counts
    for task in ("bbox", "segm"):
        for name in ("d_img", "d_cat", "d_score", "d_area", "d_row", "g_img", "g_cat", "g_area", "g_crowd", "g_col", "iou"):
            assert np.array_equal(t_crops[task].cat(name), t_planes[task].cat(name)), (task, name)
            assert np.array_equal(t_planes[task].cat(name), t_off[task].cat(name)), (task, name)
    # crowd regions are never matched, every pair has the threshold's IoU, and nobody is matched twice
    crowd = [k for k, a in enumerate(rec["annotations"]) if a["iscrowd"]]
    assert len(crowd) == 3 and not {r[4] for r in r_crops.rows} & set(crowd)
    assert all(r[6] >= ONE_IOU for r in r_crops.rows)
    assert len({r[3] for r in r_crops.rows}) == len(r_crops.rows) == len({r[4] for r in r_crops.rows})
    # an image without a pair costs no copy and launches nothing: a threshold no pair reaches
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", spy)
        copies[0] = 0
        none = CE.OutlineReport(1.0, TOLERANCE)
        score(cset, none)
        assert copies[0] == copies_off and none.rows == []
