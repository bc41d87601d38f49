"""Host side of the evaluate task's crop scoring (``evaluation.score_frame: crops``): the setting and its refusals, the room
rule of the polygon rasteriser against ``coco_ref.fr_poly``, and the host packing of run-length ground truth against
``rle_decode`` plus a NumPy pack.  Nothing here touches the GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest
import yaml

sys.path.insert(0, str(Path(__file__).resolve().parent))
import coco_ref as R  # noqa: E402
import coco_ref_ext as X  # noqa: E402


# ---- the setting ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def cfgdir(tmp_path, monkeypatch):
    from deepemia_amd.utils import config as C

    (tmp_path / "datasets").mkdir()
    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(tmp_path))
    monkeypatch.delenv("DEEPEMIA_EVAL_MODE", raising=False)

    def write(global_eval=None, ds_eval=None, mask_frame=None):
        base = {"paths": {}, "inference_settings": {"confidence_mode": "auto"}}
        if global_eval is not None:
            base["evaluation"] = global_eval
        ds = {"inference_overrides": {"confidence_mode": "auto"}}
        if mask_frame is not None:
            ds["inference_overrides"]["mask_frame"] = mask_frame
        if ds_eval is not None:
            ds["evaluation"] = ds_eval
        (tmp_path / "config.yaml").write_text(yaml.safe_dump(base))
        (tmp_path / "datasets" / "ds.yaml").write_text(yaml.safe_dump(ds))
        C.reset_cache()

    yield write
    C.reset_cache()


def test_score_frame_default_and_both_values(cfgdir):
    from deepemia_amd.functions.evaluate_model import SCORE_FRAMES, evaluation_settings, score_frame_setting
    from deepemia_amd.functions.inference import PipelineSettings

    assert SCORE_FRAMES == ("planes", "crops")
    cfgdir()
    assert score_frame_setting("ds") == "planes" and score_frame_setting() == "planes"
    assert score_frame_setting("ds", "full") == "planes"
    assert evaluation_settings("ds") == ("predictor", [1, 10, 100])          # (what existing callers unpack is unchanged)
    assert PipelineSettings("ds").score_frame == "planes"
    cfgdir(ds_eval={"score_frame": "crops", "mode": "pipeline", "max_dets": [1, 10, 500]}, mask_frame="crop_direct")
    assert score_frame_setting("ds") == "crops"
    assert score_frame_setting("ds", "crop") == "crops" and score_frame_setting("ds", "crop_direct") == "crops"
    assert evaluation_settings("ds") == ("pipeline", [1, 10, 500])
    assert PipelineSettings("ds").score_frame == "crops"
    cfgdir(global_eval={"score_frame": "crops"})                                 # the global key, next to mode and max_dets
    assert score_frame_setting("ds") == "crops" and score_frame_setting() == "crops"
    cfgdir(global_eval={"score_frame": "crops"}, ds_eval={"score_frame": "planes"})
    assert score_frame_setting("ds") == "planes"


def test_score_frame_refusals_in_both_directions_and_unknown_value(cfgdir, tmp_path):
    from deepemia_amd.functions.evaluate_model import PipelineRunner, evaluation_settings, score_frame_setting

    # crops needs a crop frame: refused before any model is looked for (the split directory does not exist)
    cfgdir(ds_eval={"score_frame": "crops"})
    with pytest.raises(ValueError, match="score_frame: crops needs inference_settings.mask_frame: crop or crop_direct"):
        PipelineRunner("ds", None, str(tmp_path / "no_models_here"), 50, 0.3)
    with pytest.raises(ValueError, match="score_frame: crops needs"):
        score_frame_setting("ds", "full")
    # planes with a crop frame: today's refusal, which now names the new key
    for frame in ("crop", "crop_direct"):
        cfgdir(mask_frame=frame)
        with pytest.raises(ValueError, match=f"^inference_settings.mask_frame: {frame} is not supported by the evaluate task.*evaluation.score_frame"):
            PipelineRunner("ds", None, str(tmp_path / "no_models_here"), 50, 0.3)
    # crops with a crop frame passes the check: the runner goes on to look for models and finds none
    cfgdir(ds_eval={"score_frame": "crops"}, mask_frame="crop")
    with pytest.raises(FileNotFoundError):
        PipelineRunner("ds", None, str(tmp_path / "no_models_here"), 50, 0.3)
    # an unknown value
    cfgdir(ds_eval={"score_frame": "rooms"}, mask_frame="crop")
    with pytest.raises(ValueError, match="score_frame must be 'planes' or 'crops', got 'rooms'"):
        score_frame_setting("ds")
    with pytest.raises(ValueError, match="score_frame must be"):
        PipelineRunner("ds", None, str(tmp_path / "no_models_here"), 50, 0.3)
    assert evaluation_settings("ds") == ("predictor", [1, 10, 100])          # the predictor mode's reader ignores the key


# ---- the room rule -----------------------------------------------------------------------------------------------------------------
def _random_polygons(rng, n, H, W):
    """Polygons inside the frame, crossing each edge, wholly outside, with a repeated vertex, with every vertex doubled;
    coordinates rounded to 0 - 12 decimals."""
    out = []
    for it in range(n):
        k = rng.randint(1, 8)
        cx, cy = rng.uniform(-10, W + 10), rng.uniform(-10, H + 10)
        sc = rng.choice([2, 10, 60])
        pts = np.round(np.stack([cx + rng.uniform(-sc, sc, k), cy + rng.uniform(-sc, sc, k)], 1), rng.choice([0, 1, 3, 6, 12]))
        if it % 5 == 0 and k > 1:
            pts[rng.randint(k)] = pts[0]
        if it % 7 == 0:
            pts = np.repeat(pts, 2, axis=0)
        if it % 11 == 0:
            pts += rng.choice([-1, 1]) * np.array([W + 80.0, 0.0]) if it % 2 else rng.choice([-1, 1]) * np.array([0.0, H + 80.0])   # wholly outside
        out.append([float(v) for v in pts.reshape(-1)])
    return out


@pytest.mark.parametrize("H,W", [(96, 200), (40, 70)])
def test_no_pixel_of_fr_poly_lies_outside_its_room(H, W):
    from deepemia_amd.cocoeval import polygon_rooms

    rng = np.random.RandomState(H)
    polys = _random_polygons(rng, 400, H, W)
    rooms = polygon_rooms([[p] for p in polys], H, W)
    assert rooms.dtype == np.int32 and rooms.shape == (400, 4)
    filled = empty_rooms = 0
    for p, (y0, x0, y1, x1) in zip(polys, rooms.tolist()):
        pos = X.runs_to_pixels(R.fr_poly(p, H, W))
        if y0 < 0:
            empty_rooms += 1
            assert len(pos) == 0, p
            continue
        assert 0 <= y0 <= y1 < H and 0 <= x0 <= x1 < W
        if len(pos):
            filled += 1
            y, x = pos % H, pos // H
            assert y.min() >= y0 and y.max() <= y1 and x.min() >= x0 and x.max() <= x1, (p, (y0, x0, y1, x1))   # no pixel outside its room
    assert filled > 100 and empty_rooms > 20                        # (the sample is not vacuous)
    ok = rooms[rooms[:, 0] >= 0]
    assert (ok[:, 0] == 0).any() and (ok[:, 1] == 0).any() and (ok[:, 2] == H - 1).any() and (ok[:, 3] == W - 1).any()   # rooms touch every frame edge
    # a mask of several polygons: one room over all of them; a mask without a polygon: empty
    both = polygon_rooms([[polys[1], polys[2]], []], H, W)
    assert both[1].tolist() == [-1] * 4
    pair = rooms[1:3][rooms[1:3, 0] >= 0]
    if len(pair) == 2:
        assert both[0].tolist() == [pair[:, 0].min(), pair[:, 1].min(), pair[:, 2].max(), pair[:, 3].max()]


def test_room_rule_values():
    from deepemia_amd.cocoeval import polygon_rooms

    rooms = polygon_rooms([[[1.5, 2.5, 10.2, 3, 5, 9.7]], [[-5, -5, -3, -5, -3, -2]], [[0.2, 0.2, 500, 0.2, 500, 300, 0.2, 300]],
                           [[68.5, 38.5, 75, 38.5, 75, 45, 68.5, 45]]], 40, 70)
    assert rooms.tolist() == [[1, 0, 10, 11], [-1, -1, -1, -1], [0, 0, 39, 69], [37, 67, 39, 69]]


# ---- run-length ground truth packed on the host ----------------------------------------------------------------------------------------
def _np_pack(mask):
    H, W = mask.shape
    wpr = (W + 31) // 32
    pad = np.zeros((H, wpr * 32), dtype=bool)
    pad[:, :W] = mask
    return np.packbits(pad.reshape(H, wpr, 32), axis=-1, bitorder="little").view(np.uint32).reshape(H, wpr)


@pytest.mark.parametrize("H,W", [(96, 200), (40, 64), (7, 33)])
def test_rle_ground_truth_packs_to_the_words_of_its_decoded_box(H, W):
    from deepemia_amd.cocoeval import rle_decode, rle_host_crop

    rng = np.random.RandomState(W)
    cases = [np.zeros((H, W), bool), np.ones((H, W), bool)]
    one = np.zeros((H, W), bool)
    one[0, 0] = True
    cases.append(one)
    one = np.zeros((H, W), bool)
    one[H - 1, W - 1] = True
    cases.append(one)
    col = np.zeros((H, W), bool)
    col[:, 3:6] = True                                                  # full columns: runs that go on into the next column
    cases.append(col)
    for _ in range(40):
        m = np.zeros((H, W), bool)
        h, w = rng.randint(1, H + 1), rng.randint(1, W + 1)
        y0, x0 = rng.randint(0, H - h + 1), rng.randint(0, W - w + 1)
        m[y0:y0 + h, x0:x0 + w] = rng.rand(h, w) < rng.choice([.1, .5, .95])
        cases.append(m)
    for m in cases:
        runs = X.encode(m)
        assert (rle_decode(runs, H, W) == m).all()
        box, words, area = rle_host_crop(runs, H, W)
        assert area == int(m.sum()) and words.dtype == np.uint32
        if area == 0:
            assert box == (-1, -1, -1, -1) and len(words) == 0
            continue
        ys, xs = np.nonzero(m)
        assert box == (ys.min(), xs.min(), ys.max(), xs.max())
        want = _np_pack(rle_decode(runs, H, W))[box[0]:box[2] + 1, box[1] >> 5:(box[3] >> 5) + 1]
        assert np.array_equal(words, want.reshape(-1))
    with pytest.raises(ValueError, match="run lengths cover"):
        rle_host_crop([0, H * W + 1], H, W)
