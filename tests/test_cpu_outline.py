"""CPU tests of the outline-agreement report: the reference's ``d2`` against SciPy's exact Euclidean distance transform on every
case, the matching function against a brute-force statement of its rule (score ties, IoU ties, crowd columns, IoU exactly at
the threshold), the rows and the summary against hand-computed values on a three-pair example, every setting's error message,
and the new entries in the header, ``_lib.EXPORTS`` and the Makefile (ABI 6)."""
import csv
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import yaml

sys.path.insert(0, str(Path(__file__).resolve().parent))
import outline_cases as OC  # noqa: E402
import outline_ref as OR  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent


# ---- the reference ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", OC.cases(), ids=lambda c: c[0])
def test_reference_d2_equals_the_distance_transform_of_the_target_border(case):
    from scipy.ndimage import distance_transform_edt

    name, det, gt, pairs = case
    for d, g in pairs.tolist():
        for src, tgt in ((det[d], gt[g]), (gt[g], det[d])):
            sp, tp = OR.points(src), OR.points(tgt)
            want = np.rint(distance_transform_edt(~OR.border(tgt)) ** 2).astype(np.int64)[sp[:, 0], sp[:, 1]]
            assert np.array_equal(OR.min_d2(sp, tp), want), (name, d, g)


def test_reference_q_and_bins():
    assert [OR.q(v) for v in (0, 1, 2, 3, 4, 9, 126 * 126, 46999 ** 2)] == [0, 256, 362, 443, 512, 768, 126 * 256, 46999 * 256]
    for v in (2, 3, 5, 15877, 2 ** 33 + 1):
        r = OR.q(v)
        assert r * r <= v << 16 < (r + 1) * (r + 1)
    assert [OR.bin_of(v) for v in (0, 1, 2, 4, 5, 9, 10, 125 * 125 + 1, 126 * 126, 126 * 126 + 1, 127 * 127, 127 * 127 + 1, 2 ** 33)] == \
        [0, 1, 2, 2, 3, 3, 4, 126, 126, 127, 127, 127, 127]
    m = np.zeros((5, 6), bool)
    m[1:4, 1:5] = True
    assert OR.border(m).sum() == 10 and not OR.border(m)[2, 2] and not OR.border(m)[2, 3]
    full = np.ones((3, 4), bool)                                      # outside the frame counts as unset
    assert OR.border(full).sum() == 10 and not OR.border(full)[1, 1]


# ---- the matching -----------------------------------------------------------------------------------------------------------------
def test_matching_equals_the_brute_force_rule_on_ties_crowds_and_the_threshold():
    from deepemia_amd import cocoeval as CE

    rng = np.random.RandomState(11)
    seen_pairs = 0
    for trial in range(200):
        D, G = rng.randint(0, 9), rng.randint(0, 9)
        thr = float(rng.choice([0.5, 0.25, 1.0]))
        iou = rng.choice([0.0, 0.25, 0.3, 0.5, 0.5, 0.75, 1.0], size=(D, G))           # few values: IoU ties, and IoU == thr
        scores = rng.choice([0.3, 0.6, 0.6, 0.9], size=D)                              # score ties
        d_cat, g_cat = rng.randint(0, 2, D), rng.randint(0, 2, G)
        crowd = (rng.rand(G) < .25).astype(np.uint8)
        got = CE.outline_match(iou, scores, d_cat, g_cat, crowd, thr)
        assert got.dtype == np.int64 and got.shape == (len(got), 2)
        assert [tuple(p) for p in got.tolist()] == OR.match(iou, scores, d_cat, g_cat, crowd, thr), trial
        assert not crowd[got[:, 1]].any() and (d_cat[got[:, 0]] == g_cat[got[:, 1]]).all()
        assert len(set(got[:, 0].tolist())) == len(got) == len(set(got[:, 1].tolist()))
        seen_pairs += len(got)
    assert seen_pairs > 200


def test_matching_known_answers():
    from deepemia_amd import cocoeval as CE

    none = np.zeros(3, np.uint8)
    # IoU exactly at the threshold pairs; just below does not
    assert CE.outline_match(np.array([[0.5, 0.49999]]), [1.0], [0], [0, 0], none[:2]).tolist() == [[0, 0]]
    assert CE.outline_match(np.array([[0.49999]]), [1.0], [0], [0], none[:1]).tolist() == []
    # the higher score chooses first; the other takes what is left; ties in score go by index
    iou = np.array([[0.9, 0.6], [0.8, 0.0]])
    assert CE.outline_match(iou, [0.5, 0.7], [0, 0], [0, 0], none[:2]).tolist() == [[0, 1], [1, 0]]
    assert CE.outline_match(iou, [0.7, 0.7], [0, 0], [0, 0], none[:2]).tolist() == [[0, 0]]
    # an IoU tie goes to the lower annotation index; a crowd column is never taken; another category neither
    assert CE.outline_match(np.array([[0.7, 0.7, 0.7]]), [1.0], [0], [0, 0, 0], none).tolist() == [[0, 0]]
    assert CE.outline_match(np.array([[0.9, 0.7, 0.6]]), [1.0], [0], [0, 0, 0], np.array([1, 0, 0], np.uint8)).tolist() == [[0, 1]]
    assert CE.outline_match(np.array([[0.9, 0.7, 0.6]]), [1.0], [1], [0, 0, 1], none).tolist() == [[0, 2]]
    # maxDets does not apply: 150 detections, 150 pairs
    assert len(CE.outline_match(np.eye(150), np.linspace(1, 0.1, 150), np.zeros(150), np.zeros(150), np.zeros(150, np.uint8))) == 150


# ---- rows and summary: three pairs by hand --------------------------------------------------------------------------------------------
def _hist(**bins):
    h = np.zeros(128, dtype=np.int64)
    for k, v in bins.items():
        h[int(k[1:])] = v
    return h


# pair A: unit distances; pair B: identical outlines; pair C: one far point in the saturating bin
RECORDS = {
    (7, 0, 0): dict(n=(4, 4), max_d2=(1, 1), sum_d2=(4, 2), sum_q=(1024, 512), hist=(_hist(b1=4), _hist(b0=2, b1=2))),
    (7, 1, 1): dict(n=(3, 3), max_d2=(0, 0), sum_d2=(0, 0), sum_q=(0, 0), hist=(_hist(b0=3), _hist(b0=3))),
    (9, 0, 0): dict(n=(10, 5), max_d2=(40000, 4), sum_d2=(40081, 20), sum_q=(58112, 2560), hist=(_hist(b3=9, b127=1), _hist(b2=5))),
}


def _three_pair_report(tolerance=0):
    from deepemia_amd import cocoeval as CE

    report = CE.OutlineReport(0.5, tolerance)
    calls = []

    def measure(image):
        def run(pairs, d_px, g_px):
            calls.append((image, pairs.tolist(), d_px.tolist(), g_px.tolist()))
            recs = [RECORDS[image, d, g] for d, g in pairs.tolist()]
            out = {k: np.asarray([r[k] for r in recs], dtype=np.int64) for k in ("n", "max_d2", "sum_d2", "sum_q")}
            out["hist"] = np.asarray([np.stack(r["hist"]) for r in recs], dtype=np.int64)
            return out
        return run
    # image 7: two pairs, a spurious detection (its only overlap is a crowd region), a missed annotation
    iou7 = np.array([[0.8, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 0.9, 0.0]])
    n7 = report.add_image(7, "a.png", [5, 8, 5], np.array([0.9, 0.8, 0.7]), [100, 50, 60], [5, 8, 5, 8], [80, 50, 70, 20], [0, 0, 1, 0], iou7, measure(7))
    # image 9: one pair, IoU exactly at the threshold
    n9 = report.add_image(9, "b.png", [5], np.array([0.6]), [314], [5], [200], [0], np.array([[0.5]]), measure(9))
    # image 11: no pair -- the device stage is not called
    n11 = report.add_image(11, "c.png", [8], np.array([0.6]), [10], [5], [10], [0], np.array([[0.9]]), None)
    assert (n7, n9, n11) == (2, 1, 0)
    assert calls == [(7, [[0, 0], [1, 1]], [100, 50, 60], [80, 50, 70, 20]), (9, [[0, 0]], [314], [200])]
    return report


def test_rows_of_the_three_pair_example():
    report = _three_pair_report()
    e_a = 2 * math.sqrt(100 / math.pi) - 2 * math.sqrt(80 / math.pi)
    e_c = 2 * math.sqrt(314 / math.pi) - 2 * math.sqrt(200 / math.pi)
    assert report.rows == [
        [7, "a.png", 5, 0, 0, 0.9, 0.8, 100, 80, 4, 4, 0.75, math.sqrt(6 / 8), 1.0, 1.0, 0.25, e_a, 0.25],
        [7, "a.png", 8, 1, 1, 0.8, 1.0, 50, 50, 3, 3, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0],
        [9, "b.png", 5, 0, 0, 0.6, 0.5, 314, 200, 10, 5, 60672 / 3840, math.sqrt(40101 / 15), 200.0, 127.0, 0.0, e_c, 114 / 200],
    ]
    # the tolerance moves NSD alone: at 3 px pair C counts its nine near points and all five of the other side
    at3 = _three_pair_report(3).rows
    assert [r[15] for r in at3] == [1.0, 1.0, 14 / 15] and [r[:15] + r[16:] for r in at3] == [r[:15] + r[16:] for r in report.rows]


def test_summary_and_files_of_the_three_pair_example(tmp_path):
    from deepemia_amd import cocoeval as CE

    report = _three_pair_report()
    e_a = 2 * math.sqrt(100 / math.pi) - 2 * math.sqrt(80 / math.pi)
    e_c = 2 * math.sqrt(314 / math.pi) - 2 * math.sqrt(200 / math.pi)
    assd_c = 60672 / 3840
    want = [
        ["pore", 3, 3, 2, 1, 1, (0.75 + assd_c) / 2, (0.75 + assd_c) / 2, 64.0, 200.0, 0.125, (e_a + e_c) / 2, (0.25 + 0.57) / 2],
        ["throat", 2, 2, 1, 1, 1, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0],
        ["void", 0, 0, 0, 0, 0] + [None] * 7,
        ["all", 5, 5, 3, 2, 2, (0.75 + 0.0 + assd_c) / 3, 0.75, 128 / 3, 200.0, 1.25 / 3, (e_a + e_c) / 3, (0.25 + 0.57) / 3],
    ]
    got = report.summary([5, 8, 9], ["pore", "throat", "void"])
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[:6] == w[:6], (g, w)
        assert all((a is None and b is None) or a == pytest.approx(b, rel=1e-15, abs=0) for a, b in zip(g[6:], w[6:])), (g, w)
    assert report.write(str(tmp_path), [5, 8, 9], ["pore", "throat", "void"]) == got
    rows = list(csv.reader(open(tmp_path / "outline_agreement.csv", newline="")))
    assert rows[0] == CE.OUTLINE_ROW_HEADER and len(rows) == 4 and all(len(r) == 19 for r in rows)
    assert rows[1][:12] == ["7", "a.png", "5", "pore", "0", "0", "0.9", "0.8", "100", "80", "4", "4"]
    assert rows[2][:4] == ["7", "a.png", "8", "throat"] and rows[3][:6] == ["9", "b.png", "5", "pore", "0", "0"]
    for text, row in zip(rows[1:], report.rows):
        assert [float(v) for v in text[6:8]] == row[5:7] and [float(v) for v in text[12:]] == row[11:]       # repr round-trips
    summ = list(csv.reader(open(tmp_path / "outline_summary.csv", newline="")))
    assert summ[0] == CE.OUTLINE_SUMMARY_HEADER and [r[0] for r in summ[1:]] == ["pore", "throat", "void", "all"]
    assert summ[3] == ["void", "0", "0", "0", "0", "0"] + [""] * 7                   # a class without a pair: empty value fields
    assert [float(v) for v in summ[4][6:]] == got[3][6:] and summ[4][1:6] == ["5", "5", "3", "2", "2"]


def test_values_from_reference_records_equal_the_reference_formulas():
    """``cocoeval.outline_values`` on the case table's records equals ``outline_ref.values``, value for value."""
    from deepemia_amd import cocoeval as CE

    name, det, gt, keep = OC.cases()[0]
    rec = OR.records(det, gt, keep)
    d_px, g_px = det.sum((1, 2))[keep[:, 0]], gt.sum((1, 2))[keep[:, 1]]
    for tol in (0, 2, 126):
        got = CE.outline_values(rec, d_px, g_px, tol)
        for k in range(len(keep)):
            want = OR.values({n: rec[n][k, 0] for n in rec}, {n: rec[n][k, 1] for n in rec}, int(d_px[k]), int(g_px[k]), tol)
            assert {n: float(got[n][k]) for n in CE.OUTLINE_VALUES} == want, (tol, k)


# ---- the setting -----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def cfgdir(tmp_path, monkeypatch):
    from deepemia_amd.utils import config as C

    (tmp_path / "datasets").mkdir()
    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(tmp_path))
    monkeypatch.delenv("DEEPEMIA_EVAL_MODE", raising=False)

    def write(global_eval=None, ds_eval=None):
        base = {"paths": {}, "inference_settings": {"confidence_mode": "auto"}}
        if global_eval is not None:
            base["evaluation"] = global_eval
        ds = {"inference_overrides": {"confidence_mode": "auto"}}
        if ds_eval is not None:
            ds["evaluation"] = ds_eval
        (tmp_path / "config.yaml").write_text(yaml.safe_dump(base))
        (tmp_path / "datasets" / "ds.yaml").write_text(yaml.safe_dump(ds))
        C.reset_cache()

    yield write
    C.reset_cache()


def test_outline_setting_default_values_and_scopes(cfgdir):
    from deepemia_amd.functions.evaluate_model import boundary_setting, evaluation_settings, outline_setting

    cfgdir()
    assert outline_setting("ds") is None and outline_setting() is None                         # off by default
    cfgdir(ds_eval={"outline_agreement": False, "outline_iou": 0.7})
    assert outline_setting("ds") is None
    cfgdir(ds_eval={"outline_agreement": True})
    assert outline_setting("ds") == (0.5, 2)
    assert boundary_setting("ds") is None and evaluation_settings("ds") == ("predictor", [1, 10, 100])      # (the other settings are untouched)
    cfgdir(global_eval={"outline_agreement": True, "outline_tolerance": 0})                    # the global key
    assert outline_setting("ds") == (0.5, 0) and outline_setting() == (0.5, 0)
    cfgdir(global_eval={"outline_agreement": True}, ds_eval={"outline_agreement": True, "outline_iou": 1, "outline_tolerance": 126})
    assert outline_setting("ds") == (1.0, 126)


@pytest.mark.parametrize("key,value,message", [
    ("outline_agreement", "yes", "evaluation.outline_agreement must be true or false, got 'yes'"),
    ("outline_agreement", 1, "evaluation.outline_agreement must be true or false, got 1"),
    ("outline_iou", "0.5", "evaluation.outline_iou must be a number in (0, 1], got '0.5'"),
    ("outline_iou", 0, "evaluation.outline_iou must be a number in (0, 1], got 0"),
    ("outline_iou", -0.5, "evaluation.outline_iou must be a number in (0, 1], got -0.5"),
    ("outline_iou", 1.01, "evaluation.outline_iou must be a number in (0, 1], got 1.01"),
    ("outline_iou", True, "evaluation.outline_iou must be a number in (0, 1], got True"),
    ("outline_tolerance", -1, "evaluation.outline_tolerance must be an integer from 0 to 126, got -1"),
    ("outline_tolerance", 127, "evaluation.outline_tolerance must be an integer from 0 to 126, got 127"),
    ("outline_tolerance", 2.0, "evaluation.outline_tolerance must be an integer from 0 to 126, got 2.0"),
    ("outline_tolerance", "2", "evaluation.outline_tolerance must be an integer from 0 to 126, got '2'"),
    ("outline_tolerance", False, "evaluation.outline_tolerance must be an integer from 0 to 126, got False"),
])
@pytest.mark.parametrize("switch", [True, False])
def test_outline_setting_errors_name_the_key_and_come_before_any_model(cfgdir, tmp_path, key, value, message, switch):
    from deepemia_amd.functions.evaluate_model import evaluate_model, outline_setting

    ev = {"outline_agreement": switch}                    # the keys are checked whether or not the switch is on
    ev[key] = value
    cfgdir(ds_eval=ev)
    with pytest.raises(ValueError, match=re.escape(message)):
        outline_setting("ds")
    # through the task's entry: raised before the paths are read or a model is looked for (this configuration has neither)
    for mode in ("predictor", "pipeline"):
        with pytest.raises(ValueError, match=re.escape(message)):
            evaluate_model("ds", str(tmp_path / "out"), rcnn=50, mode=mode)
    assert not (tmp_path / "out").exists()


# ---- the entries -----------------------------------------------------------------------------------------------------------------
def test_entries_in_header_exports_and_makefile_with_abi_6():
    from deepemia_amd import _lib

    header = (ROOT / "include" / "deepemia_hip.h").read_text()
    csrc = ROOT / "deepemia_amd" / "csrc"
    for name in ("demia_mask_outline_agreement", "demia_crop_outline_agreement", "demia_outline_source_share", "demia_outline_target_tile"):
        assert name in _lib.EXPORTS and f"int {name}(" in header
    assert "int64_t demia_outline_chunks(" in header and _lib.EXPORTS["demia_outline_chunks"][0] is _lib.C.c_int64
    assert len(_lib.EXPORTS["demia_mask_outline_agreement"][1]) == 22 and len(_lib.EXPORTS["demia_crop_outline_agreement"][1]) == 26
    assert "int demia_abi_version(void) { return 6; }" in (csrc / "capi.hip").read_text()
    assert re.search(r"^SRCS\s*=.*\boutline\.hip\b", (csrc / "Makefile").read_text(), re.M)
    src = (csrc / "outline.hip").read_text()
    for name in ("demia_mask_outline_agreement", "demia_crop_outline_agreement", "demia_outline_chunks"):
        assert 'extern "C"' in src and f" {name}(" in src
    # one border kernel, in the shared header; the definitions are stated in the public header
    assert "void mask_border_kernel(" not in src and '#include "maskborder.h"' in src
    for phrase in ("q(d2)  = isqrt(d2 << 16)", "bin(d2) = min(127, the smallest integer c with c * c >= d2)", "unset 4-neighbour",
                   "SATURATES", "The CALLER zeroes out"):
        assert phrase in header, phrase
    if _lib.LIB_PATH.exists():
        lib = _lib.load()
        assert lib.demia_abi_version() == 6
        tile, share = lib.demia_outline_target_tile(), lib.demia_outline_source_share()
        assert tile >= 4 and tile % 4 == 0 and share >= 1
        # the sizer is host code: ceil(pixels of the source / share) workgroups per pair-direction, at least 1, at most 256
        d_area, g_area = np.asarray([0, share + 1], dtype=np.int64), np.asarray([1000 * share], dtype=np.int64)
        pairs = np.asarray([[0, 0], [1, 0]], dtype=np.int32)
        off = np.zeros(5, dtype=np.int64)
        assert lib.demia_outline_chunks(d_area.ctypes.data, 2, g_area.ctypes.data, 1, pairs.ctypes.data, 2, off.ctypes.data) == 515
        assert off.tolist() == [0, 1, 257, 259, 515]
