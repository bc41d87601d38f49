"""Host side of the crop-framed mask sets: the ``mask_frame`` setting and the room / offset computation of the placement."""
import numpy as np
import pytest
import yaml


# ------------------------------------------------------------------------------------------------------------ configuration
def _settings(tmp_path, monkeypatch, overrides):
    from deepemia_amd.functions.inference import PipelineSettings
    from deepemia_amd.utils import config as C
    (tmp_path / "datasets").mkdir(exist_ok=True)
    (tmp_path / "config.yaml").write_text(yaml.safe_dump({"paths": {}, "inference_settings": {"confidence_mode": "auto"}}))
    (tmp_path / "datasets" / "ds.yaml").write_text(yaml.safe_dump({"inference_overrides": overrides}))
    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(tmp_path))
    C.reset_cache()
    try:
        return PipelineSettings("ds")
    finally:
        C.reset_cache()


def test_mask_frame_defaults_to_full(tmp_path, monkeypatch):
    from deepemia_amd.functions.inference import mask_frame_setting
    assert mask_frame_setting({}) == "full" and mask_frame_setting(None) == "full"
    assert _settings(tmp_path, monkeypatch, {"tile_settings": {"tile_size": 256}}).mask_frame == "full"


def test_mask_frame_is_read_per_dataset(tmp_path, monkeypatch):
    assert _settings(tmp_path, monkeypatch, {"mask_frame": "crop"}).mask_frame == "crop"
    assert _settings(tmp_path, monkeypatch, {"mask_frame": "full", "merge_mode": "soft_nms"}).mask_frame == "full"


def test_unknown_mask_frame_is_a_configuration_error(tmp_path, monkeypatch):
    with pytest.raises(ValueError, match="mask_frame must be 'full' or 'crop'"):
        _settings(tmp_path, monkeypatch, {"mask_frame": "cropped"})


@pytest.mark.parametrize("extra, word", [({"merge_mode": "soft_nms"}, "soft_nms"), ({"multiscale_settings": {"enabled": True}}, "multiscale")])
def test_crop_with_the_modes_that_stay_on_full_is_refused(tmp_path, monkeypatch, extra, word):
    with pytest.raises(ValueError, match=word):
        _settings(tmp_path, monkeypatch, dict({"mask_frame": "crop"}, **extra))
    from deepemia_amd.functions.inference import mask_frame_setting
    assert mask_frame_setting(dict({"mask_frame": "full"}, **extra)) == "full"          # ... and allowed on the default frame


def test_crop_with_more_than_one_rank_is_refused_at_start(monkeypatch):
    import types
    import torch.distributed as dist
    from deepemia_amd.functions.inference import InferencePipeline
    fake = types.SimpleNamespace(engine=types.SimpleNamespace(device="cpu"))
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda: 1)
    monkeypatch.setattr(dist, "get_world_size", lambda: 2)
    with pytest.raises(ValueError, match="one process only"):
        InferencePipeline([fake], "t", {"mask_frame": "crop"}, {})
    assert InferencePipeline([fake], "t", {"mask_frame": "full"}, {}).mask_frame == "full"


# -------------------------------------------------------------------------------------------------------- rooms and offsets
def _restated_rooms(boxes, src_hw, tile_hw, xo, yo, hw):
    """The placement restated on dense arrays: the box as a mask, cv2's INTER_NEAREST index rule, the paste, the clip."""
    (sh, sw), (th, tw), (H, W) = src_hw, tile_hw, hw
    iy = np.minimum(np.floor(np.arange(th) * (1.0 / (th / sh))).astype(int), sh - 1)
    ix = np.minimum(np.floor(np.arange(tw) * (1.0 / (tw / sw))).astype(int), sw - 1)
    out = []
    for (y0, x0, y1, x1), dx, dy in zip(boxes, xo, yo):
        frame = np.zeros((H, W), bool)
        if y0 >= 0:
            m = np.zeros((sh, sw), bool)
            m[y0:y1 + 1, x0:x1 + 1] = True
            t = m[iy][:, ix]
            ye, xe = min(dy + th, H), min(dx + tw, W)
            frame[dy:ye, dx:xe] = t[:ye - dy, :xe - dx]
        ys, xs = np.nonzero(frame)
        out.append([-1] * 4 if len(ys) == 0 else [ys.min(), xs.min(), ys.max(), xs.max()])
    return np.asarray(out, dtype=np.int32)


@pytest.mark.parametrize("s", [128, 64, 96, 50])
def test_rooms_equal_the_restated_placement_of_the_boxes(s):
    from deepemia_amd.cropset import rooms_of_placed_tiles
    g = np.random.default_rng(s)
    n, H, W, T = 300, 96, 200, 64
    y0, x0 = g.integers(0, s, n), g.integers(0, s, n)
    boxes = np.stack([y0, x0, np.minimum(y0 + g.integers(0, s // 2, n), s - 1), np.minimum(x0 + g.integers(0, s // 2, n), s - 1)], axis=1)
    boxes[::17] = -1
    boxes[1] = (0, 0, s - 1, s - 1)
    xo = g.choice([0, 150, 136, 37, 199], n)
    yo = g.choice([0, 50, 32, 11, 95], n)
    got = rooms_of_placed_tiles(boxes, (s, s), (T, T), xo, yo, (H, W))
    assert got.dtype == np.int32 and np.array_equal(got, _restated_rooms(boxes, (s, s), (T, T), xo, yo, (H, W)))
    assert (got[:, 0] < 0).sum() > n // 17 and (got[:, 3] == W - 1).any() and (got[:, 2] == H - 1).any()


def test_offsets_are_the_exclusive_prefix_sums_of_rows_times_word_columns():
    from deepemia_amd.cropset import room_lengths, room_offsets
    room = np.array([[0, 0, 0, 0], [-1, -1, -1, -1], [3, 31, 5, 32], [10, 64, 10, 199], [0, 0, 95, 199]], dtype=np.int32)
    assert room_lengths(room).tolist() == [1, 0, 6, 5, 96 * 7]
    offs, total = room_offsets(room)
    assert offs.dtype == np.int64 and offs.tolist() == [0, 1, 1, 7, 12] and total == 12 + 96 * 7
    assert room_offsets(np.zeros((0, 4), np.int32))[1] == 0


def test_evaluate_pipeline_mode_refuses_crop_before_loading_models(tmp_path, monkeypatch):
    """The evaluate task's pipeline mode scores full-frame planes: a dataset with ``mask_frame: crop`` is a configuration error there."""
    from deepemia_amd.functions.evaluate_model import PipelineRunner
    from deepemia_amd.utils import config as C
    (tmp_path / "datasets").mkdir()
    (tmp_path / "config.yaml").write_text(yaml.safe_dump({"paths": {}, "inference_settings": {"confidence_mode": "auto"}}))
    (tmp_path / "datasets" / "ds.yaml").write_text(yaml.safe_dump({"inference_overrides": {"mask_frame": "crop"}}))
    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(tmp_path))
    C.reset_cache()
    try:
        with pytest.raises(ValueError, match="mask_frame: crop is not supported by the evaluate task"):
            PipelineRunner("ds", None, str(tmp_path / "no_models_here"), 50, 0.3)
    finally:
        C.reset_cache()
