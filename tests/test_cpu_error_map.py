"""CPU tests of the error maps of ``--task evaluate --visualize``: the dense reference (``error_map_ref``) against a hand-computed
scene and against its own invariants on every scene of ``error_map_cases``, the setting's parsing and refusals, the states derived
from ``cocoeval.outline_match``, the rows, the CSV text and the file names of ``cocoeval.ErrorMaps`` with a stub ``paint``, the
default line rule, and the entries in the header, the exports and the Makefile."""
import csv
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import yaml
from PIL import Image

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(Path(__file__).resolve().parent))
import error_map_cases as EC  # noqa: E402
import error_map_ref as ER  # noqa: E402


# ---- the reference ----------------------------------------------------------------------------------------------------------------
def test_reference_on_a_hand_computed_scene():
    """6 x 6, gray 100, alpha 128, line 1.  The detection (matched) is rows 0-4 x columns 0-3, the annotation (matched) rows 1-5 x
    columns 1-5.  Eroded by 3 x 3 with the outside unset: rows 1-3 x columns 1-2 and rows 2-4 x columns 2-4.  Y: the detection's
    outline, W: the annotation's where the detection's is not, g / b: the agree / missing fill left between them, '.': the base."""
    hw = (6, 6)
    det, gt = np.zeros((1,) + hw, dtype=bool), np.zeros((1,) + hw, dtype=bool)
    det[0, 0:5, 0:4] = True
    gt[0, 1:6, 1:6] = True
    src = np.full(hw, 100, dtype=np.uint8)
    dst, counts = ER.error_map(det, [1], gt, [1], src, 128, 1)
    colour = {"Y": (0, 255, 255), "W": (255, 255, 255), "g": (50, 178, 50), "b": (178, 50, 50), ".": (100, 100, 100)}
    want = ["YYYY..",
            "YWWYWW",
            "YWgYbW",
            "YWgYbW",
            "YYYYbW",
            ".WWWWW"]
    assert dst.dtype == np.uint8 and dst.shape == (6, 6, 3)
    for y, row in enumerate(want):
        for x, ch in enumerate(row):
            assert tuple(dst[y, x]) == colour[ch], (y, x, ch, tuple(dst[y, x]))
    assert counts.tolist() == [12, 8, 13, 0] and counts.dtype == np.int64
    # the detection unmatched, the annotation a crowd region: what they share is ignored, the rest of the detection excess, nothing is missing
    dst, counts = ER.error_map(det, [2], gt, [3], src, 256, 1)
    assert counts.tolist() == [0, 8, 0, 12]
    assert tuple(dst[2, 2]) == (100, 100, 100)            # ignored: not filled
    assert tuple(dst[0, 0]) == (255, 0, 255) and tuple(dst[5, 5]) == (128, 128, 128) and tuple(dst[1, 3]) == (255, 0, 255)
    assert tuple(dst[3, 4]) == (100, 100, 100)            # inside the crowd region alone: the base


SCENES = EC.scenes()


def test_scenes_cover_what_the_kernel_can_get_wrong():
    rows, words, per_round = EC.parse_tile()
    assert rows * words == per_round                        # one thread per word of a tile
    sizes = EC.frame_sizes()
    assert sorted(w % 32 for _, w in sizes) == [0, 6, 31]
    for H, W in sizes:
        assert H > 2 * rows and H % rows and W > 2 * 32 * words and (W + 31) // 32 > 2 * words and ((W + 31) // 32) % words
    assert {s.image.shape[2] for s in SCENES} == {1, 3} and {0, 96, 256} <= {s.alpha for s in SCENES}
    assert {s.line for s in SCENES} == {1, 2, 3, 4} and {s.palette is None for s in SCENES} == {True, False}
    assert {(len(s.det) == 0, len(s.gt) == 0) for s in SCENES} == {(False, False), (True, False), (False, True), (True, True)}
    by = {s.name: s for s in SCENES}
    # more masks on one tile than one ballot round takes, of each set
    crowded = by["crowded_tile"]
    for m in (crowded.det, crowded.gt):
        ys, xs = np.nonzero(m.any(axis=0))
        assert len(m) > per_round and ys.max() < rows and 32 * words <= xs.min() and xs.max() < 2 * 32 * words
    # masks thinner than the line for every width, and the first that are not
    for t in (1, 2, 3, 4):
        s = by[f"thin_t{t}"]
        thin = [ER.outline(m, t).sum() == m.sum() for m in s.det]
        assert s.line == t and thin == [True] * (2 * t) + [False] * 2
    # the seams: a mask on both sides of a tile seam each way and of a word seam; the edges; the column W - 1; a pixel; empty; full
    for s in SCENES[:3]:
        H, W = s.hw
        both = np.concatenate([s.det, s.gt])
        assert any(m[rows - 1].any() and m[rows].any() and m[:, 32 * words - 1].any() and m[:, 32 * words].any() for m in both)
        assert any(m[:, 31].any() and m[:, 32].any() for m in both)
        assert all(any(e(m).any() and not m.all() for m in both) for e in (lambda m: m[0], lambda m: m[-1], lambda m: m[:, 0], lambda m: m[:, -1]))
        assert any(m.sum() == 1 for m in both) and any(m.all() for m in both) and any(not m.any() for m in both)
        assert any(m.all() and st == 0 for m, st in zip(s.det, s.d_state))


@pytest.mark.parametrize("scene", SCENES + [EC.random_scene(k) for k in range(4)], ids=lambda s: s.name)
def test_reference_invariants(scene):
    s = scene
    agree, ignored, excess, missing = ER.fill_classes(s.det, s.d_state, s.gt, s.g_state, s.hw)
    stack = np.stack([agree, ignored, excess, missing]).astype(int)
    assert stack.sum(axis=0).max() <= 1                     # disjoint
    dall, gall = ER.union(s.det, s.d_state, (1, 2), s.hw), ER.union(s.gt, s.g_state, (1, 2), s.hw)
    dst, counts = ER.error_map(s.det, s.d_state, s.gt, s.g_state, s.image, s.alpha, s.line, s.palette)
    assert counts.tolist() == [int(agree.sum()), int(excess.sum()), int(missing.sum()), int(ignored.sum())]
    # the four classes tile Dall | Gall: agree + excess + missing is |Dall | Gall| less the ignored pixels, which the fourth count adds
    assert int(counts.sum()) == int((dall | gall).sum()) and int(counts[:3].sum()) + int(ignored.sum()) == int((dall | gall).sum())
    # alpha = 0 leaves only outlines: away from them the picture is the base
    dst0, counts0 = ER.error_map(s.det, s.d_state, s.gt, s.g_state, s.image, 0, s.line, s.palette)
    lines = np.any(ER.line_classes(s.det, s.d_state, s.gt, s.g_state, s.line, s.hw), axis=0)
    assert np.array_equal(dst0[~lines], ER.base_image(s.image)[~lines]) and np.array_equal(counts0, counts)
    pal = ER.PALETTE if s.palette is None else s.palette
    assert all(any(np.array_equal(px, c) for c in pal[3:]) for px in dst0[lines][:50])
    # the order of the masks within a state means nothing
    rng = np.random.RandomState(3)
    pd, pg = rng.permutation(len(s.det)), rng.permutation(len(s.gt))
    again, counts2 = ER.error_map(s.det[pd], s.d_state[pd], s.gt[pg], s.g_state[pg], s.image, s.alpha, s.line, s.palette)
    assert np.array_equal(again, dst) and np.array_equal(counts2, counts)


def test_reference_palette_is_the_default_table():
    from deepemia_amd import cocoeval as CE

    assert np.array_equal(np.asarray(CE.ERROR_MAP_PALETTE, dtype=np.uint8), ER.PALETTE)
    assert len(CE.ERROR_MAP_LABELS) == 8
    # green, red, blue, magenta, cyan, yellow, white, mid-grey -- as BGR
    assert CE.ERROR_MAP_PALETTE == ((0, 255, 0), (0, 0, 255), (255, 0, 0), (255, 0, 255), (255, 255, 0), (0, 255, 255), (255, 255, 255), (128, 128, 128))
    # the one table: no other file of the package states the colours
    for path in (ROOT / "deepemia_amd").rglob("*.py"):
        if path.name != "cocoeval.py":
            assert "(255, 0, 255), (255, 255, 0)" not in path.read_text(), path


# ---- the setting ------------------------------------------------------------------------------------------------------------------
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


def test_visualize_setting_defaults_values_and_scopes(cfgdir):
    from deepemia_amd.functions.evaluate_model import boundary_setting, outline_setting, visualize_setting

    cfgdir()
    assert visualize_setting("ds") == (0.5, 96, None) == visualize_setting()
    cfgdir(ds_eval={"visualize_iou": 1, "visualize_alpha": 0, "visualize_line": 4})
    got = visualize_setting("ds")
    assert got == (1.0, 0, 4) and [type(v) for v in got] == [float, int, int]
    assert boundary_setting("ds") is None and outline_setting("ds") is None                  # (the other settings are untouched)
    cfgdir(global_eval={"visualize_alpha": 256, "visualize_line": 1})                          # the global key
    assert visualize_setting("ds") == (0.5, 256, 1) == visualize_setting()
    cfgdir(global_eval={"visualize_alpha": 256}, ds_eval={"visualize_iou": 0.25})
    assert visualize_setting("ds")[0] == 0.25


@pytest.mark.parametrize("key,value,message", [
    ("visualize_iou", "0.5", "evaluation.visualize_iou must be a number in (0, 1], got '0.5'"),
    ("visualize_iou", 0, "evaluation.visualize_iou must be a number in (0, 1], got 0"),
    ("visualize_iou", -0.5, "evaluation.visualize_iou must be a number in (0, 1], got -0.5"),
    ("visualize_iou", 1.01, "evaluation.visualize_iou must be a number in (0, 1], got 1.01"),
    ("visualize_iou", True, "evaluation.visualize_iou must be a number in (0, 1], got True"),
    ("visualize_alpha", -1, "evaluation.visualize_alpha must be an integer from 0 to 256, got -1"),
    ("visualize_alpha", 257, "evaluation.visualize_alpha must be an integer from 0 to 256, got 257"),
    ("visualize_alpha", 96.0, "evaluation.visualize_alpha must be an integer from 0 to 256, got 96.0"),
    ("visualize_alpha", "96", "evaluation.visualize_alpha must be an integer from 0 to 256, got '96'"),
    ("visualize_alpha", True, "evaluation.visualize_alpha must be an integer from 0 to 256, got True"),
    ("visualize_line", 0, "evaluation.visualize_line must be an integer from 1 to 4, got 0"),
    ("visualize_line", 5, "evaluation.visualize_line must be an integer from 1 to 4, got 5"),
    ("visualize_line", 2.0, "evaluation.visualize_line must be an integer from 1 to 4, got 2.0"),
    ("visualize_line", "auto", "evaluation.visualize_line must be an integer from 1 to 4, got 'auto'"),
    ("visualize_line", False, "evaluation.visualize_line must be an integer from 1 to 4, got False"),
])
@pytest.mark.parametrize("flag", [True, False])
def test_visualize_setting_errors_name_the_key_and_come_before_any_model(cfgdir, tmp_path, key, value, message, flag):
    from deepemia_amd.functions.evaluate_model import evaluate_model, visualize_setting

    cfgdir(ds_eval={key: value})
    with pytest.raises(ValueError, match=re.escape(message)):
        visualize_setting("ds")
    # through the task's entry, whether or not the flag is given: raised before the paths are read or a model is looked for
    for mode in ("predictor", "pipeline"):
        with pytest.raises(ValueError, match=re.escape(message)):
            evaluate_model("ds", str(tmp_path / "out"), visualize=flag, rcnn=50, mode=mode)
    assert not (tmp_path / "out").exists()


# ---- states, rows, files ----------------------------------------------------------------------------------------------------------
def test_default_line_rule():
    from deepemia_amd import cocoeval as CE

    want = {(1, 1): 1, (512, 512): 1, (1024, 300): 1, (1536, 100): 2, (100, 1537): 2, (2048, 2048): 2, (2560, 1): 2, (2561, 1): 3,
            (3072, 3072): 3, (3584, 10): 4, (4096, 4096): 4, (8192, 8192): 4, (65535, 65535): 4}
    for (H, W), t in want.items():
        assert CE.error_map_line(H, W) == t == min(4, max(1, round(max(H, W) / 1024))), (H, W)
    maps = CE.ErrorMaps("out")
    assert (maps.iou, maps.alpha, maps.line) == (0.5, 96, None) and maps.line_for(2048, 100) == 2
    assert CE.ErrorMaps("out", 0.3, 10, 3).line_for(8192, 8192) == 3


def _image_inputs():
    """Five detections against six annotations (the last a crowd region): by the matching rule detection 0 (the higher score) takes
    annotation 1, detection 1 annotation 0; detection 2 has the wrong class, 3 is below the threshold, 4 meets the crowd region alone."""
    iou = np.zeros((5, 6))
    iou[0, 1], iou[0, 0], iou[1, 0], iou[1, 1] = .8, .6, .7, .9
    iou[2, 2] = .9
    iou[3, 3] = .49
    iou[4, 5] = .95
    scores = np.asarray([.9, .8, .7, .6, .5])
    d_cat, g_cat = np.asarray([0, 0, 1, 0, 0]), np.asarray([0, 0, 0, 0, 1, 0])
    crowd = np.asarray([0, 0, 0, 0, 0, 1])
    return iou, scores, d_cat, g_cat, crowd


def test_states_come_from_outline_match():
    from deepemia_amd import cocoeval as CE

    iou, scores, d_cat, g_cat, crowd = _image_inputs()
    pairs = CE.outline_match(iou, scores, d_cat, g_cat, crowd, 0.5)
    assert pairs.tolist() == [[0, 1], [1, 0]]
    d_state, g_state = CE.error_map_states(pairs, 5, crowd)
    assert d_state.tolist() == [1, 1, 2, 2, 2] and g_state.tolist() == [1, 1, 2, 2, 2, 3]
    assert d_state.dtype == np.int32 and g_state.dtype == np.int32
    d_state, g_state = CE.error_map_states(np.zeros((0, 2), np.int64), 0, np.zeros(0))
    assert d_state.shape == (0,) and g_state.shape == (0,)
    d_state, g_state = CE.error_map_states(CE.outline_match(iou, scores, d_cat, g_cat, crowd, 0.85), 5, crowd)
    assert d_state.tolist() == [2, 1, 2, 2, 2] and g_state.tolist() == [2, 1, 2, 2, 2, 3]


def test_error_maps_rows_csv_and_file_names(tmp_path):
    from deepemia_amd import cocoeval as CE

    iou, scores, d_cat, g_cat, crowd = _image_inputs()
    maps = CE.ErrorMaps(str(tmp_path / "out"), 0.5, 96, 2)
    assert not (tmp_path / "out").exists()                  # nothing is written before an image is added
    seen = []
    picture = np.random.RandomState(0).randint(0, 256, (7, 9, 3)).astype(np.uint8)

    def paint(counts):
        def run(d_state, g_state):
            seen.append((d_state.tolist(), g_state.tolist()))
            return picture, np.asarray(counts, dtype=np.int64)
        return run
    # two images with the same base name in different folders, one image without anything
    p0 = maps.add_image(7, "a/x/em.tif", d_cat, scores, g_cat, crowd, iou, paint([30, 10, 20, 5]))
    p1 = maps.add_image(8, "b/y/em.tif", d_cat[:0], scores[:0], g_cat[:0], crowd[:0], np.zeros((0, 0)), paint([0, 0, 0, 0]))
    p2 = maps.add_image("id9", "plain.png", d_cat[:1], scores[:1], g_cat[:0], crowd[:0], np.zeros((1, 0)), paint([0, 4, 0, 0]))
    assert seen == [([1, 1, 2, 2, 2], [1, 1, 2, 2, 2, 3]), ([], []), ([2], [])]
    images = tmp_path / "out" / "evaluation_images"
    assert [Path(p) for p in (p0, p1, p2)] == [images / "7_em_evaluation.png", images / "8_em_evaluation.png", images / "id9_plain_evaluation.png"]
    for p in (p0, p1, p2):                                  # BGR on the device, RGB in the file
        assert np.array_equal(np.asarray(Image.open(p).convert("RGB")), picture[:, :, ::-1])
    table = maps.write()
    assert Path(table) == tmp_path / "out" / "evaluation_images.csv"
    text = Path(table).read_text()
    rows = list(csv.reader(text.splitlines()))
    assert rows[0] == CE.ERROR_MAP_HEADER == ["image_id", "file_name", "detections", "annotations", "matched", "missed", "spurious", "crowd",
                                              "agree_px", "excess_px", "missing_px", "ignored_px", "pixel_precision", "pixel_recall", "pixel_dice"]
    assert rows[1] == ["7", "em.tif", "5", "5", "2", "3", "3", "1", "30", "10", "20", "5", repr(30 / 40), repr(30 / 50), repr(60 / 90)]
    assert rows[2] == ["8", "em.tif", "0", "0", "0", "0", "0", "0", "0", "0", "0", "0", "", "", ""]          # no denominator: empty fields
    assert rows[3] == ["id9", "plain.png", "1", "0", "0", "0", "1", "0", "0", "4", "0", "0", repr(0.0), "", repr(0.0)]
    assert [float(v) for v in rows[1][12:]] == [0.75, 0.6, 60 / 90]
    legend = Image.open(images / "legend.png").convert("RGB")
    colours = {c for _, c in legend.getcolors(1 << 16)}
    assert all((r, g, b) in colours for b, g, r in CE.ERROR_MAP_PALETTE) and legend.size[1] >= 8 * 12
    assert sorted(p.name for p in images.iterdir()) == ["7_em_evaluation.png", "8_em_evaluation.png", "id9_plain_evaluation.png", "legend.png"]


# ---- the entries ------------------------------------------------------------------------------------------------------------------
def test_entries_in_header_exports_and_makefile():
    from deepemia_amd import _lib

    header = (ROOT / "include" / "deepemia_hip.h").read_text()
    csrc = ROOT / "deepemia_amd" / "csrc"
    for name in ("demia_mask_error_map", "demia_crop_error_map"):
        assert name in _lib.EXPORTS and f"int {name}(" in header and _lib.EXPORTS[name][0] is _lib.C.c_int
    assert "int64_t demia_error_map_tiles(" in header and _lib.EXPORTS["demia_error_map_tiles"][0] is _lib.C.c_int64
    assert len(_lib.EXPORTS["demia_mask_error_map"][1]) == 19 and len(_lib.EXPORTS["demia_crop_error_map"][1]) == 23
    assert re.search(r"^SRCS\s*=.*\berrormap\.hip\b", (csrc / "Makefile").read_text(), re.M)
    src = (csrc / "errormap.hip").read_text()
    for name in ("demia_mask_error_map", "demia_crop_error_map", "demia_error_map_tiles"):
        assert 'extern "C"' in src and f" {name}(" in src
    # one kernel over a word source, on the shared reductions; no atomics, no floating point
    assert src.count("void error_map_kernel(") == 1 and "template <class S>" in src and "wreg::block_sum" in src and "mwords::word_at" in src
    assert not re.search(r"\batomic\w*\(|\bfloat\b|\bdouble\b", src)
    for phrase in ("outline_t(m) = m \\ erode_t(m)", "(b_c * (256 - alpha) + colour_c * alpha + 128) >> 8", "counted and NOT filled",
                   "Bits of mask words beyond column W - 1 are nobody's pixels"):
        assert phrase in header, phrase
    if _lib.LIB_PATH.exists():
        lib = _lib.load()
        rows, words, _ = EC.parse_tile()
        for H, W in EC.frame_sizes() + [(1, 1), (rows, 32 * words), (rows + 1, 32 * words + 1), (65535, 65535)]:
            assert lib.demia_error_map_tiles(H, W) == -(-H // rows) * -(-((W + 31) // 32) // words), (H, W)
        assert lib.demia_error_map_tiles(0, 5) == 0
