"""CPU tests of the boundary-AP feature: the two reference statements of the band agree on every case of the table, known
answers, the width rule, the settings' errors, and the new entries in the header, ``_lib.EXPORTS`` and the Makefile (ABI 6)."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import yaml

sys.path.insert(0, str(Path(__file__).resolve().parent))
import boundary_cases as BC  # noqa: E402
import boundary_ref as BR  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent


# ---- the reference statements --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", BC.FRAMES)
def test_window_and_published_construction_agree_on_every_case(H, W):
    for d in BC.widths(H, W):
        names, dense = BC.masks(H, W, d)
        for m0 in range(0, len(dense), 16):
            want = BR.eroded(dense[m0:m0 + 16], d)
            got = BR.eroded_published(dense[m0:m0 + 16], d)
            bad = np.nonzero((want != got).reshape(len(want), -1).any(axis=1))[0]
            assert len(bad) == 0, (d, [names[m0 + b] for b in bad])


@pytest.mark.parametrize("H,W", [f for f in BC.FRAMES if f[0] * f[1] <= 40 * 65])
def test_summed_area_statement_is_the_literal_window(H, W):
    for d in (1, 2, 3):
        names, dense = BC.masks(H, W, d)
        for name, m in list(zip(names, dense))[::3]:
            assert np.array_equal(BR.eroded(m, d), BR.eroded_literal(m, d)), (d, name)
    rng = np.random.RandomState(H * W)
    for _ in range(20):
        m = rng.rand(H, W) < rng.choice([.7, .9, .97, 1.0])
        d = int(rng.randint(1, 8))
        assert np.array_equal(BR.eroded(m, d), BR.eroded_literal(m, d))
        assert np.array_equal(BR.eroded_published(m, d), BR.eroded_literal(m, d))


def test_the_table_covers_its_edges():
    names, dense = BC.masks(640, 640, 58)
    assert (640 * 20 > BC.LARGE_WORDS) and dense[names.index("full")].all()                  # the global-scratch path
    assert BR.eroded(dense, 58)[[names.index(n) for n in names if n.startswith("blob_")]].any()      # blobs wide enough to keep a core
    for H, W in BC.FRAMES:
        for d in BC.widths(H, W):
            names, dense = BC.masks(H, W, d)
            assert len(names) == len(set(names)) == len(dense) and sum(n.startswith("blob_") for n in names) == 64
    assert BC.widths(70, 100)[-1] > 100 and BC.widths(640, 640) == (1, 58)
    names, dense = BC.masks(70, 100, 3)
    sq = dense[names.index("square_7")]
    assert BR.tight_box(sq) == [1, 28, 7, 34]                                               # across the bit-31 / 32 boundary


# ---- known answers ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3, 5])
def test_a_square_erodes_to_its_core_and_the_band_keeps_the_box(d):
    for k in (2 * d, 2 * d + 1, 2 * d + 2, 2 * d + 9):
        m = np.zeros((40, 70), dtype=bool)
        m[3:3 + k, 30:30 + k] = True
        e = BR.eroded(m, d)
        assert e.sum() == max(0, k - 2 * d) ** 2
        b = BR.band(m, d)
        assert BR.tight_box(b) == BR.tight_box(m) and not (b & ~m).any()
        assert b.sum() == k * k - max(0, k - 2 * d) ** 2
        if k <= 2 * d:
            assert np.array_equal(b, m)                                                    # thinner than 2d + 1: its own band
    full = np.ones((20, 30), dtype=bool)                                                   # the frame's ring of width d
    b = BR.band(full, d)
    assert b.sum() == 20 * 30 - (20 - 2 * d) * (30 - 2 * d) and b[:d].all() and b[:, :d].all() and not b[d:-d, d:-d].any()


def test_boundary_iou_known_answers():
    from deepemia_amd import cocoeval as CE

    a = np.zeros((40, 40), dtype=bool)
    a[5:25, 5:25] = True
    far = np.zeros_like(a)
    far[30:38, 30:38] = True
    assert BR.boundary_iou(a, a, 2) == 1.0 and BR.boundary_iou(a, far, 2) == 0.0
    # a 20 x 20 square against itself moved 3 px to the right, d = 1: each band is the square's 1-px ring, 20^2 - 18^2 = 76 pixels.
    # The rings share their top and bottom rows over the 17 common columns 8 .. 24 and nothing else: a's right side (column 24) and
    # g's left side (column 8) run through the other square's interior.  34 / (76 + 76 - 34).
    g = np.zeros_like(a)
    g[5:25, 8:28] = True
    lit = 34
    assert BR.band(a, 1).sum() == 76 and BR.band(g, 1).sum() == 76 and np.count_nonzero(BR.band(a, 1) & BR.band(g, 1)) == lit
    assert BR.boundary_iou(a, g, 1) == 34 / 118
    assert BR.mask_iou(a, g) == 340 / 460 and min(BR.mask_iou(a, g), BR.boundary_iou(a, g, 1)) == 34 / 118
    # the crowd denominator is the detection's band
    assert BR.boundary_iou(a, g, 1, crowd=True) == 34 / 76
    # cocoeval.boundary_iou is mask_iou on the band counts
    got = CE.boundary_iou(np.array([[lit, 0]]), np.array([76]), np.array([76, 28]), np.array([0, 0]))
    assert got.tolist() == [[lit / (152 - lit), 0.0]]
    got = CE.boundary_iou(np.array([[lit, 0]]), np.array([76]), np.array([76, 28]), np.array([1, 1]))
    assert got.tolist() == [[lit / 76, 0.0]]


# ---- the width rule --------------------------------------------------------------------------------------------------------------
def test_boundary_width_rule():
    from deepemia_amd import cocoeval as CE

    assert CE.BOUNDARY_RATIO == 0.02
    assert CE.boundary_width(2048, 2048) == 58 and CE.boundary_width(8192, 8192) == 232 and CE.boundary_width(512, 512) == 14
    assert CE.boundary_width(10, 10) == 1 and CE.boundary_width(1, 1) == 1 and CE.boundary_width(30, 40, 0.001) == 1      # the floor
    assert CE.boundary_width(30, 40, 0.05) == 2 and CE.boundary_width(30, 40, 0.07) == 4                   # round(2.5) = 2: half to even
    assert CE.boundary_width(2048, 2048, 0.02, 7) == 7 and CE.boundary_width(5, 5, width=300) == 300       # pixels given: no ratio
    for bad in (0, -3, 2.0, "2", True):
        with pytest.raises(ValueError, match="integer >= 1"):
            CE.boundary_width(100, 100, 0.02, bad)


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


def test_boundary_setting_default_values_and_scopes(cfgdir):
    from deepemia_amd.functions.evaluate_model import _new_tables, boundary_setting, evaluation_settings

    cfgdir()
    assert boundary_setting("ds") is None and boundary_setting() is None                       # off by default
    assert list(_new_tables(None)) == ["bbox", "segm"]
    cfgdir(ds_eval={"boundary_ap": False, "boundary_width": 3})
    assert boundary_setting("ds") is None
    cfgdir(ds_eval={"boundary_ap": True})
    assert boundary_setting("ds") == (0.02, None)
    assert list(_new_tables(boundary_setting("ds"))) == ["bbox", "segm", "boundary"]
    assert evaluation_settings("ds") == ("predictor", [1, 10, 100])                            # (what existing callers unpack is unchanged)
    cfgdir(global_eval={"boundary_ap": True, "boundary_dilation_ratio": 0.01})                 # the global key
    assert boundary_setting("ds") == (0.01, None) and boundary_setting() == (0.01, None)
    cfgdir(global_eval={"boundary_ap": True}, ds_eval={"boundary_ap": True, "boundary_width": 2, "boundary_dilation_ratio": 0.05})
    assert boundary_setting("ds") == (0.05, 2)


@pytest.mark.parametrize("key,value,message", [
    ("boundary_ap", "yes", "evaluation.boundary_ap must be true or false, got 'yes'"),
    ("boundary_ap", 1, "evaluation.boundary_ap must be true or false, got 1"),
    ("boundary_dilation_ratio", "0.02", "evaluation.boundary_dilation_ratio must be a number"),
    ("boundary_dilation_ratio", 0, "evaluation.boundary_dilation_ratio must be a number"),
    ("boundary_dilation_ratio", -0.1, "evaluation.boundary_dilation_ratio must be a number"),
    ("boundary_dilation_ratio", 1.5, "evaluation.boundary_dilation_ratio must be a number"),
    ("boundary_dilation_ratio", True, "evaluation.boundary_dilation_ratio must be a number"),
    ("boundary_width", 0, "evaluation.boundary_width must be an integer >= 1, got 0"),
    ("boundary_width", -2, "evaluation.boundary_width must be an integer >= 1"),
    ("boundary_width", 2.5, "evaluation.boundary_width must be an integer >= 1"),
    ("boundary_width", "3", "evaluation.boundary_width must be an integer >= 1"),
    ("boundary_width", True, "evaluation.boundary_width must be an integer >= 1"),
])
def test_boundary_setting_errors_name_the_key_and_come_before_any_model(cfgdir, tmp_path, key, value, message):
    from deepemia_amd.functions.evaluate_model import boundary_setting, evaluate_model

    ev = {"boundary_ap": True}
    ev[key] = value
    cfgdir(ds_eval=ev)
    with pytest.raises(ValueError, match=re.escape(message)):
        boundary_setting("ds")
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
    for name in ("demia_mask_boundary_band", "demia_crop_boundary_band"):
        assert name in _lib.EXPORTS and f"int {name}(" in header
    assert "int64_t demia_crop_boundary_scratch(" in header and _lib.EXPORTS["demia_crop_boundary_scratch"][0] is _lib.C.c_int64
    assert len(_lib.EXPORTS["demia_mask_boundary_band"][1]) == 10 and len(_lib.EXPORTS["demia_crop_boundary_band"][1]) == 13
    assert len(_lib.EXPORTS["demia_crop_boundary_scratch"][1]) == 5
    assert "int demia_abi_version(void) { return 6; }" in (csrc / "capi.hip").read_text()
    assert re.search(r"^SRCS\s*=.*\bboundary\.hip\b", (csrc / "Makefile").read_text(), re.M)
    src = (csrc / "boundary.hip").read_text()
    for name in ("demia_mask_boundary_band", "demia_crop_boundary_scratch", "demia_crop_boundary_band"):
        assert f'extern "C"' in src and f" {name}(" in src
    # the definitions are stated in the header: width, eroded mask, band, the task's IoU
    for phrase in ("max(1, int(round(ratio * sqrt(H*H + W*W))))", "band(m, d) = m & ~eroded(m, d)", "min(mask IoU, bIoU)",
                   "The CALLER zeroes"):
        assert phrase in header, phrase
    if _lib.LIB_PATH.exists():
        lib = _lib.load()
        assert lib.demia_abi_version() == 6
        # the sizer is host code: rooms of 8192 words get nothing, 8193 and more their own words; empty rooms nothing
        room = np.array([[0, 0, 255, 1023], [-1, -1, -1, -1], [0, 0, 256, 1023], [10, 31, 10, 32], [0, 5, 639, 639]], dtype=np.int32)
        off = np.zeros(5, dtype=np.int64)
        total = lib.demia_crop_boundary_scratch(room.ctypes.data, 5, 2048, 2048, off.ctypes.data)
        assert off.tolist() == [0, 0, 0, 257 * 32, 257 * 32] and total == 257 * 32 + 640 * 20
