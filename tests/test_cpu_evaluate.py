"""CPU tests of the evaluate task: the rasteriser restatement on analytic cases, the split rule, the RLE string codec, the
native COCOeval matching + numpy accumulate on hand-built IoU tables, the test-split dicts and the CLI's refusals."""
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import coco_ref as R  # noqa: E402


# ---- rasteriser restatement ------------------------------------------------------------------------------------------------
def test_fr_poly_rectangle_with_half_pixel_shift():
    # the reference's +0.5 shift: a rectangle with corners (x0, y0) .. (x1, y1) covers columns x0 + 1 .. x1, rows y0 + 1 .. y1
    h, w = 8, 10
    for x0, y0, x1, y1 in [(2, 1, 6, 4), (0, 0, 9, 7), (3, 3, 4, 4), (-3, -2, 2, 3)]:
        poly = [x0 + .5, y0 + .5, x1 + .5, y0 + .5, x1 + .5, y1 + .5, x0 + .5, y1 + .5]
        want = np.zeros((h, w), bool)
        want[max(y0 + 1, 0):y1 + 1, max(x0 + 1, 0):x1 + 1] = True
        assert (R.poly_mask([poly], h, w) == want).all(), (x0, y0, x1, y1)
    # unshifted integer corners: columns x0 .. x1 - 1, rows y0 .. y1 - 1 (pycocotools' pixel-centre rule)
    m = R.poly_mask([[2, 1, 6, 1, 6, 4, 2, 4]], h, w)
    want = np.zeros((h, w), bool)
    want[1:4, 2:6] = True
    assert (m == want).all()


def test_fr_poly_triangle():
    m = R.poly_mask([[1, 1, 8, 1, 1, 6]], 8, 10).astype(int)
    want = np.array([[0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                     [0, 1, 1, 1, 1, 1, 1, 0, 0, 0],
                     [0, 1, 1, 1, 1, 1, 0, 0, 0, 0],
                     [0, 1, 1, 1, 0, 0, 0, 0, 0, 0],
                     [0, 1, 1, 0, 0, 0, 0, 0, 0, 0],
                     [0, 1, 0, 0, 0, 0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
                     [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]])
    assert (m == want).all()


def test_fr_poly_below_bottom_edge_carries_into_next_column():
    h, w = 8, 10
    # a rectangle cut by the bottom edge: the boundary clamped to y = h closes each column's run at row 0 of the next
    counts = R.fr_poly([2.5, 3.5, 5.5, 3.5, 5.5, 20, 2.5, 20], h, w)
    assert counts == [28, 4, 4, 4, 4, 4, 32]
    want = np.zeros((h, w), bool)
    want[4:, 3:6] = True
    assert (R.decode(counts, h, w) == want).all()
    # a triangle whose crossing points do not pair up inside each column: the parity runs on over the column-major order
    xy = [5.3, 10.1, 7.7, 10.2, 5.6, 4.6]
    m = R.poly_mask([xy], h, w)
    want = np.zeros((h, w), bool)
    want[7, 5:7] = True
    assert (m == want).all()
    pos = np.cumsum(R.fr_poly(xy, h, w))[:-1]
    assert any(p % h == 0 and p > 0 for p in pos)       # a toggle at row 0 of a column: the clamped y = h of the one before


def test_fr_poly_degenerate_rings():
    h, w = 8, 10
    assert R.fr_poly([3, 3], h, w) == [h * w]                      # one vertex
    assert R.fr_poly([3, 3, 3, 3, 3, 3], h, w) == [h * w]          # all vertices equal
    assert R.fr_poly([1, 1, 5, 1], h, w) == [h * w]                # a segment
    assert R.fr_poly([], h, w) == [h * w]
    # a repeated closing vertex (the 65-point ellipse ring) is a zero-length edge: no effect on a convex ring
    sq = [1.5, 1.5, 5.5, 1.5, 5.5, 5.5, 1.5, 5.5]
    assert R.fr_poly(sq + sq[:2], h, w) == R.fr_poly(sq, h, w)


# ---- split rule ----------------------------------------------------------------------------------------------------------------
def test_split_rule_known_listing(tmp_path):
    from deepemia_amd.data.datasets import load_or_create_split, split_rule

    files = [f"{c}.json" for c in "abcdefghij"]
    train, test = split_rule(files)
    # train_test_split(range(10), test_size=0.2, random_state=42): test [8, 1], train [5, 0, 7, 2, 9, 4, 3, 6]
    assert test == ["i.json", "b.json"]
    assert train == [f"{c}.json" for c in "fahcjedg"]
    assert (train, test) == R.split_rule(files)
    assert split_rule(list(range(7)))[1] == list(np.random.RandomState(42).permutation(7)[:2])
    img = tmp_path / "imgs"
    img.mkdir()
    for f in reversed(files):
        (img / f).write_text("{}")
    (img / "x.png").write_bytes(b"")
    data = load_or_create_split(str(img), "ds", tmp_path / "split")
    assert data == {"train": train, "test": test}
    assert json.loads((tmp_path / "split" / "ds_split.json").read_text()) == data
    (tmp_path / "split" / "ds_split.json").write_text(json.dumps({"train": [], "test": ["a.json"]}))
    assert load_or_create_split(str(img), "ds", tmp_path / "split")["test"] == ["a.json"]


def test_split_dicts_follow_the_reference(tmp_path):
    from deepemia_amd.data.datasets import ellipse_polygon, get_split_dicts

    lab = {"metadata": {"name": "a.tif", "height": 40, "width": 50},
           "instances": [{"type": "polygon", "className": "pore", "points": [1, 2, 11, 2, 11, 9, 1, 9]},
                         {"type": "polygon", "className": "nope", "points": [1, 2, 3, 4, 5, 6]},
                         {"type": "ellipse", "className": "throat", "cx": 20, "cy": 15, "rx": 6.7, "ry": 3.2, "angle": 30}]}
    (tmp_path / "a.json").write_text(json.dumps(lab))
    recs = get_split_dicts("imgs", str(tmp_path), ["a.json"], ["pore", "throat"])
    assert len(recs) == 1 and recs[0]["image_id"] == 0 and recs[0]["file_name"].endswith("a.tif")
    a0, a1 = recs[0]["annotations"]
    assert a0["category_id"] == 0 and a0["segmentation"] == [[1.5, 2.5, 11.5, 2.5, 11.5, 9.5, 1.5, 9.5]]
    assert [float(v) for v in a0["bbox"]] == [1, 2, 11, 9] and a0["area"] == 70.0
    px, py = ellipse_polygon(20, 15, 6.7, 3.2, 30)
    assert len(px) == 65 and px[0] == px[-1] and py[0] == py[-1]
    assert a1["category_id"] == 1 and len(a1["segmentation"][0]) == 130
    assert a1["segmentation"][0][:2] == [px[0] + .5, py[0] + .5]
    # scaled by (int(rx), int(ry)) = (6, 3) and rotated 30 degrees about the centre: every vertex on that ellipse
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    dx, dy = px - 20, py - 15
    u, v = c * dx + s * dy, -s * dx + c * dy
    assert np.allclose((u / 6) ** 2 + (v / 3) ** 2, 1.0)
    assert abs(a1["area"] - 0.5 * 64 * math.sin(2 * math.pi / 64) * 18) < 1e-3


# ---- RLE strings ---------------------------------------------------------------------------------------------------------------
def test_rle_string_hand_checked_and_round_trip():
    from deepemia_amd import cocoeval as CE

    assert CE.rle_strings(np.array([3, 5, 100], np.uint32), np.array([0, 3]))[0] == "35T3"
    assert CE.rle_strings(np.array([3, 5, 100, 2], np.uint32), np.array([0, 4]))[0] == "35T3M"      # 2 - 5 = -3 -> 'M'
    assert R.to_string([3, 5, 100, 2]) == "35T3M"
    rng = np.random.RandomState(3)
    lists = [list(rng.randint(0, 5000, size=rng.randint(1, 40))) for _ in range(30)] + [[0, 7, 1 << 30], [262144]]
    counts = np.concatenate([np.asarray(c, np.uint32) for c in lists])
    off = np.concatenate([[0], np.cumsum([len(c) for c in lists])])
    got = CE.rle_strings(counts, off)
    for c, s in zip(lists, got):
        assert s == R.to_string(c)
        assert list(CE.rle_from_string(s)) == [int(v) for v in c]
        assert R.from_string(s) == [int(v) for v in c]


# ---- scoring on hand-built IoU tables ------------------------------------------------------------------------------------------
def _score(images, names=("a", "b")):
    """images: list of (dets [(cat, score, area)], gts [(cat, area, crowd)], iou [D, G]) -> derive_results of the segm task."""
    from deepemia_amd import cocoeval as CE

    t = CE.EvalTables()
    for i, (dets, gts, iou) in enumerate(images):
        t.add_image(i, [d[0] for d in dets], [d[1] for d in dets], [d[2] for d in dets], [g[0] for g in gts],
                    [g[1] for g in gts], [g[2] for g in gts], np.asarray(iou, np.float64).reshape(len(dets), len(gts)))
    ev = CE.evaluate({"segm": t}, list(range(len(images))), list(range(len(names))))["segm"]
    return CE.derive_results(ev["stats"], ev["precision"], list(names)), ev


def test_perfect_detection_gives_ap_100():
    res, ev = _score([([(0, .9, 5000)], [(0, 5000, 0)], [[1.0]])], names=("a",))
    # precision is tp / (tp + fp + eps): a perfect ranking scores 100 / (1 + 2^-52), as pycocotools'
    for k in ("AP", "AP50", "AP75", "APm", "AP-a"):
        assert res[k] == pytest.approx(100, abs=1e-9)
    assert math.isnan(res["APs"]) and math.isnan(res["APl"])
    assert ev["stats"][8] == 1.0                                    # AR@100


def test_one_box_at_iou_062():
    res, _ = _score([([(0, .9, 5000)], [(0, 5000, 0)], [[0.62]])], names=("a",))
    assert res["AP50"] == pytest.approx(100, abs=1e-9) and res["AP75"] == 0
    assert res["AP"] == pytest.approx(30, abs=1e-9)                               # matched at 0.50, 0.55, 0.60 of ten thresholds


def test_higher_scored_false_positive():
    # ranked: FP (0.9), TP (0.8): precision [0, 1/2] -> monotone [1/2, 1/2] at every recall point -> AP 50
    res, _ = _score([([(0, .9, 5000), (0, .8, 5000)], [(0, 5000, 0)], [[0.0], [1.0]])], names=("a",))
    assert abs(res["AP"] - 50) < 1e-9 and abs(res["AP-a"] - 50) < 1e-9
    # the other order: AP 100
    res, _ = _score([([(0, .8, 5000), (0, .9, 5000)], [(0, 5000, 0)], [[0.0], [1.0]])], names=("a",))
    assert res["AP"] == pytest.approx(100, abs=1e-9)


def test_class_without_ground_truth_is_nan_and_no_medium_is_nan():
    res, _ = _score([([(0, .9, 500), (1, .7, 500)], [(0, 500, 0)], [[1.0, ], [0.0]])])
    assert res["AP-a"] == pytest.approx(100, abs=1e-9) and math.isnan(res["AP-b"])
    assert res["APs"] == pytest.approx(100, abs=1e-9) and math.isnan(res["APm"]) and math.isnan(res["APl"])


def test_crowd_region_is_ignored_and_matched_many_times():
    # gts: a regular object and a crowd region; dets: two inside the crowd (higher scores) and the true one
    dets = [(0, .95, 3000), (0, .9, 3000), (0, .5, 5000)]
    gts = [(0, 5000, 0), (0, 20000, 1)]
    iou = [[0.0, 0.97], [0.0, 0.99], [1.0, 0.0]]
    res, _ = _score([(dets, gts, iou)], names=("a",))
    assert res["AP"] == pytest.approx(100, abs=1e-9)                                          # both crowd matches are ignored, not false positives
    res, _ = _score([(dets, [(0, 5000, 0), (0, 20000, 0)], iou)], names=("a",))
    assert res["AP"] < 99                                           # the same region as a regular object: one FP ranks first
    # a crowd region alone: nothing to recall -> nan
    res, _ = _score([([(0, .9, 3000)], [(0, 20000, 1)], [[0.9]])], names=("a",))
    assert math.isnan(res["AP"])


def test_native_matching_equals_the_restated_cocoeval():
    """Random IoU tables through the native match + numpy accumulate against coco_ref's loop-by-loop COCOeval."""
    from deepemia_amd import cocoeval as CE

    rng = np.random.RandomState(0)
    for trial in range(3):
        images, gts, dts = [], [], []
        t = CE.EvalTables()
        tabs = {}
        for i in range(4):
            G, D = rng.randint(0, 6), rng.randint(0, 12)
            gl = [(int(rng.randint(0, 3)), float(rng.choice([300, 2000, 12000])), int(rng.rand() < .15)) for _ in range(G)]
            dl = [(int(rng.randint(0, 3)), float(np.float32(rng.choice([.5, .6, .7, .8, .9]) if rng.rand() < .3 else rng.rand())),
                   float(rng.choice([300, 2000, 12000]))) for _ in range(D)]
            iou = np.where(rng.rand(D, G) < .5, rng.rand(D, G), 0.0)
            t.add_image(i, [d[0] for d in dl], [d[1] for d in dl], [d[2] for d in dl], [g[0] for g in gl], [g[1] for g in gl],
                        [g[2] for g in gl], iou)
            images.append({"id": i, "height": 10, "width": 10})
            base_g = len(gts)
            for j, g in enumerate(gl):
                gts.append({"id": base_g + j + 1, "image_id": i, "category_id": g[0], "iscrowd": g[2], "area": g[1], "col": j})
            for k, d in enumerate(dl):
                dts.append({"image_id": i, "category_id": d[0], "score": d[1], "bbox": [0, 0, 1, 1], "row": k, "a": d[2]})
            tabs[i] = iou
        ev = CE.evaluate({"segm": t}, [im["id"] for im in images], [0, 1, 2])["segm"]
        stats, prec = _ref_on_tables(images, gts, dts, tabs)
        assert np.array_equal(ev["precision"], prec)
        assert np.array_equal(ev["stats"], stats)


def _ref_on_tables(images, gts, dts, tabs):
    """coco_ref.coco_eval with the given tables as its IoU step and the given detection areas."""
    return R.coco_eval(images, gts, dts, [0, 1, 2], "segm", iou_lookup=lambda d, g: tabs[d["image_id"]][d["row"], g["col"]],
                       dt_area=lambda d: d["a"])


# ---- CLI ------------------------------------------------------------------------------------------------------------------------
def test_cli_refusals(monkeypatch):
    import main as cli

    assert cli.main(["--task", "evaluate", "--dataset_name", "x", "--rcnn", "combo", "--no-gpu-check"]) == 2
    assert cli.main(["--task", "evaluate", "--no-gpu-check"]) == 2
    assert cli.main(["--task", "train", "--dataset_name", "x", "--no-gpu-check"]) == 2
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert cli.main(["--task", "evaluate", "--dataset_name", "x", "--rcnn", "50", "--no-gpu-check"]) == 2
