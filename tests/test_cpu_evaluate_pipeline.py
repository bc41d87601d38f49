"""CPU tests of the evaluate task's pipeline mode: COCOeval at a configurable ``maxDets``, the mask-tight box rule
(``toBbox`` of the run lengths) and the ``evaluation`` configuration key with its environment override."""
import sys
from pathlib import Path

import numpy as np
import pytest
import yaml

sys.path.insert(0, str(Path(__file__).resolve().parent))
import coco_ref as R  # noqa: E402
import coco_ref_ext as X  # noqa: E402


# ---- maxDets -------------------------------------------------------------------------------------------------------------------
def _random_tables(rng, n_images=4, max_g=6, max_d=12):
    from deepemia_amd import cocoeval as CE

    images, gts, dts, tabs = [], [], [], {}
    t = CE.EvalTables()
    for i in range(n_images):
        G, D = rng.randint(0, max_g), rng.randint(0, max_d)
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
    return t, images, gts, dts, tabs


def _lookup(tabs):
    return dict(iou_lookup=lambda d, g: tabs[d["image_id"]][d["row"], g["col"]], dt_area=lambda d: d["a"])


@pytest.mark.parametrize("max_dets", [None, [1, 10, 100], [1, 10, 1000], [2, 5, 7]])
def test_max_dets_on_random_tables(max_dets):
    """The default and an explicit [1, 10, 100] are today's function bit for bit (= ``coco_ref.coco_eval``, as the existing
    test demands of it); any other maxDets equals ``coco_ref``'s loops run at that maxDets."""
    from deepemia_amd import cocoeval as CE

    rng = np.random.RandomState(11)
    for _ in range(3):
        t, images, gts, dts, tabs = _random_tables(rng, max_d=30)
        ids = [im["id"] for im in images]
        ev = (CE.evaluate({"segm": t}, ids, [0, 1, 2]) if max_dets is None else CE.evaluate({"segm": t}, ids, [0, 1, 2], max_dets))["segm"]
        if max_dets in (None, [1, 10, 100]):
            stats, prec = R.coco_eval(images, gts, dts, [0, 1, 2], "segm", **_lookup(tabs))
            assert CE.summary_lines(ev["stats"], max_dets) == CE.summary_lines(ev["stats"])
        else:
            stats, prec = X.coco_eval(images, gts, dts, [0, 1, 2], "segm", max_dets, **_lookup(tabs))
        assert np.array_equal(ev["precision"], prec)
        assert np.array_equal(ev["stats"], stats)
        assert np.array_equal(CE.summarize(ev["precision"], ev["recall"], max_dets), stats)


def test_extended_reference_is_the_reference_at_the_default():
    rng = np.random.RandomState(5)
    _, images, gts, dts, tabs = _random_tables(rng)
    a = R.coco_eval(images, gts, dts, [0, 1, 2], "segm", **_lookup(tabs))
    b = X.coco_eval(images, gts, dts, [0, 1, 2], "segm", [1, 10, 100], **_lookup(tabs))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_300_perfect_detections_need_max_dets_above_100():
    """One image, 300 ground truths, 300 detections that match them exactly: AR@1000 = 1 and AP = 1 at maxDets [1, 10, 1000];
    at the default the best 100 are all that count, AR@100 = 100 / 300."""
    from deepemia_amd import cocoeval as CE

    n = 300
    rng = np.random.RandomState(3)
    scores = rng.permutation(n).astype(np.float64) / n * .5 + .5           # distinct
    iou = np.eye(n)
    t = CE.EvalTables()
    t.add_image(0, np.zeros(n, int), scores, np.full(n, 2000.0), np.zeros(n, int), np.full(n, 2000.0), np.zeros(n, np.uint8), iou)
    images = [{"id": 0, "height": 10, "width": 10}]
    gts = [{"id": j + 1, "image_id": 0, "category_id": 0, "iscrowd": 0, "area": 2000.0, "col": j} for j in range(n)]
    dts = [{"image_id": 0, "category_id": 0, "score": float(scores[k]), "bbox": [0, 0, 1, 1], "row": k, "a": 2000.0} for k in range(n)]
    look = _lookup({0: iou})
    big = CE.evaluate({"segm": t}, [0], [0], [1, 10, 1000])["segm"]
    assert big["stats"][8] == 1.0                                            # AR@1000
    # (AR is numpy's mean over the ten IoU thresholds of ten equal recalls: equal to the recall to an ulp)
    assert big["stats"][6] == pytest.approx(1 / n, abs=1e-15) and big["stats"][7] == pytest.approx(10 / n, abs=1e-15)      # AR@1, AR@10
    assert big["stats"][0] == pytest.approx(1.0, abs=1e-12)
    stats, prec = X.coco_eval(images, gts, dts, [0], "segm", [1, 10, 1000], **look)
    assert np.array_equal(big["stats"], stats) and np.array_equal(big["precision"], prec)
    assert " maxDets=1000 ]" in CE.summary_lines(big["stats"], [1, 10, 1000])[0]
    small = CE.evaluate({"segm": t}, [0], [0])["segm"]
    assert small["stats"][8] == pytest.approx(100 / n, abs=1e-15)            # AR@100
    assert np.all(small["recall"][:, 0, 0, 2] == 100 / n) and np.all(big["recall"][:, 0, 0, 2] == 1.0)
    stats, prec = R.coco_eval(images, gts, dts, [0], "segm", **look)
    assert np.array_equal(small["stats"], stats) and np.array_equal(small["precision"], prec)


def test_malformed_max_dets_is_refused():
    from deepemia_amd import cocoeval as CE

    for bad in ([1, 10], [10, 1, 100], [0, 10, 100], [1, 10, 10]):
        with pytest.raises(ValueError):
            CE.check_max_dets(bad)


# ---- the box of a pipeline detection ---------------------------------------------------------------------------------------------
def _box_cases(h, w):
    def m():
        return np.zeros((h, w), bool)
    cases = {"empty": m()}
    a = m(); a[3:7, 4:9] = True; cases["inside"] = a
    a = m(); a[0, 5:8] = True; cases["top edge"] = a
    a = m(); a[h - 1, 2:4] = True; cases["bottom edge"] = a
    a = m(); a[2:5, 0] = True; cases["left edge"] = a
    a = m(); a[6:9, w - 1] = True; cases["right edge"] = a
    a = m(); a[0, 0] = True; a[h - 1, w - 1] = True; cases["two corners"] = a
    a = m(); a[:, :] = True; cases["full"] = a
    a = m(); a[h - 1, 4] = True; a[0, 5] = True; cases["run across a column end"] = a      # toBbox spans all rows
    a = m(); a[:, 3:6] = True; cases["full columns"] = a
    a = m(); a[h - 1, 4] = True; a[1, 5] = True; cases["bottom then second row"] = a       # no run across: tight
    return cases


def test_box_rule_is_tobbox_of_the_run_lengths():
    from deepemia_amd import cocoeval as CE

    h, w = 11, 13
    cases = _box_cases(h, w)
    rng = np.random.RandomState(4)
    for i in range(20):
        cases[f"random {i}"] = rng.rand(h, w) < rng.choice([.02, .3])
    runs = [R.encode(v) for v in cases.values()]
    counts = np.concatenate([np.asarray(r, np.uint32) for r in runs])
    off = np.concatenate([[0], np.cumsum([len(r) for r in runs])])
    got = CE.rle_to_bbox(counts, off, h)
    assert got.dtype == np.float64 and got.shape == (len(cases), 4)
    for (name, mask), r, g in zip(cases.items(), runs, got):
        assert list(g) == X.to_bbox(r, h, w), name
        assert X.encode(mask) == r, name
        ys, xs = np.nonzero(mask)
        crossing = len(ys) and bool((mask[h - 1, :-1] & mask[0, 1:]).any())
        if not len(ys):
            assert list(g) == [0, 0, 0, 0], name
        elif not crossing:                                          # the tight box of the pixels
            assert list(g) == [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1], name
        else:
            assert list(g) == [xs.min(), 0, xs.max() - xs.min() + 1, h], name
    assert list(cases["run across a column end"].nonzero()[0]) == [0, h - 1]
    assert CE.rle_to_bbox(np.zeros(0, np.uint32), np.zeros(1, np.int64), h).shape == (0, 4)


def test_cross_counts_helper_equals_einsum():
    rng = np.random.RandomState(8)
    d, g = rng.rand(7, 9, 12) < .3, rng.rand(5, 9, 12) < .3
    di, dp = np.nonzero(d.reshape(7, -1))
    gi, gp = np.nonzero(g.reshape(5, -1))
    want = np.einsum("dp,gp->dg", d.reshape(7, -1).astype(int), g.reshape(5, -1).astype(int))
    assert np.array_equal(X.cross_counts((di, dp), (gi, gp), 7, 5), want)


# ---- configuration ---------------------------------------------------------------------------------------------------------------
def _config_tree(root, glob=None, per_dataset=None):
    (root / "datasets").mkdir(parents=True, exist_ok=True)
    base = {"bucket": None, "paths": {"split_dir": str(root / "split"), "category_json": str(root / "info.json"), "local_dataset_root": str(root)}}
    if glob is not None:
        base["evaluation"] = glob
    (root / "config.yaml").write_text(yaml.safe_dump(base))
    if per_dataset is not None:
        (root / "datasets" / "ds.yaml").write_text(yaml.safe_dump({"evaluation": per_dataset}))
    elif (root / "datasets" / "ds.yaml").exists():
        (root / "datasets" / "ds.yaml").unlink()


@pytest.fixture
def settings(tmp_path, monkeypatch):
    from deepemia_amd.functions.evaluate_model import evaluation_settings
    from deepemia_amd.utils import config as C

    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(tmp_path))
    monkeypatch.delenv("DEEPEMIA_EVAL_MODE", raising=False)

    def read(glob=None, per_dataset=None):
        _config_tree(tmp_path, glob, per_dataset)
        C.reset_cache()
        try:
            return evaluation_settings("ds")
        finally:
            C.reset_cache()
    yield read
    C.reset_cache()


def test_evaluation_key_and_environment_override(settings, monkeypatch):
    assert settings() == ("predictor", [1, 10, 100])                                   # nothing is required
    assert settings({"mode": "pipeline"}) == ("pipeline", [1, 10, 100])               # global
    assert settings({"max_dets": [1, 10, 1000]}) == ("predictor", [1, 10, 1000])
    assert settings({"mode": "predictor", "max_dets": [1, 10, 500]}, {"mode": "pipeline"}) == ("pipeline", [1, 10, 500])      # per dataset, merged
    monkeypatch.setenv("DEEPEMIA_EVAL_MODE", "predictor")
    assert settings({"mode": "pipeline"})[0] == "predictor"
    monkeypatch.setenv("DEEPEMIA_EVAL_MODE", "pipeline")
    assert settings()[0] == "pipeline"
    monkeypatch.setenv("DEEPEMIA_EVAL_MODE", "tiles")
    with pytest.raises(ValueError):
        settings()
    monkeypatch.delenv("DEEPEMIA_EVAL_MODE")
    with pytest.raises(ValueError):
        settings({"mode": "whole"})
    with pytest.raises(ValueError):
        settings({"max_dets": [100]})


def test_cli_refuses_an_unknown_mode_and_keeps_its_refusals(tmp_path, monkeypatch):
    import main as cli
    from deepemia_amd.utils import config as C

    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(tmp_path))
    monkeypatch.setenv("DEEPEMIA_OFFLINE", "1")
    monkeypatch.delenv("DEEPEMIA_EVAL_MODE", raising=False)
    _config_tree(tmp_path, {"mode": "whole"})
    C.reset_cache()
    try:
        assert cli.main(["--task", "evaluate", "--dataset_name", "ds", "--rcnn", "50", "--no-gpu-check"]) == 2
        monkeypatch.setenv("DEEPEMIA_EVAL_MODE", "nonsense")
        _config_tree(tmp_path)
        C.reset_cache()
        assert cli.main(["--task", "evaluate", "--dataset_name", "ds", "--rcnn", "50", "--no-gpu-check"]) == 2
        # predictor mode (set or by default) still refuses the model pair; several processes are refused in both modes
        monkeypatch.setenv("DEEPEMIA_EVAL_MODE", "predictor")
        assert cli.main(["--task", "evaluate", "--dataset_name", "ds", "--rcnn", "combo", "--no-gpu-check"]) == 2
        monkeypatch.delenv("DEEPEMIA_EVAL_MODE")
        assert cli.main(["--task", "evaluate", "--dataset_name", "ds", "--rcnn", "combo", "--no-gpu-check"]) == 2
        monkeypatch.setenv("WORLD_SIZE", "2")
        for mode in ("predictor", "pipeline"):
            monkeypatch.setenv("DEEPEMIA_EVAL_MODE", mode)
            assert cli.main(["--task", "evaluate", "--dataset_name", "ds", "--rcnn", "combo", "--no-gpu-check"]) == 2
    finally:
        C.reset_cache()


def test_evaluate_model_refuses_an_unknown_mode_and_combo_in_predictor_mode(tmp_path):
    from deepemia_amd.functions.evaluate_model import evaluate_model

    with pytest.raises(ValueError):
        evaluate_model("ds", str(tmp_path), mode="whole")
    with pytest.raises(ValueError):
        evaluate_model("ds", str(tmp_path), rcnn="combo")
