"""``inference_settings.detections_per_image`` (Detectron2's ``TEST.DETECTIONS_PER_IMAGE``) without a device: the setting's
default, range and error text, the dataset file overriding the global one, ``_cfg`` carrying the value, and the engine's
own range check."""
import pytest
import yaml


def test_setting_default_range_and_error_text():
    from deepemia_amd.functions.inference import detections_per_image_setting

    assert detections_per_image_setting({}) == 100 and detections_per_image_setting(None) == 100
    assert detections_per_image_setting({"detections_per_image": 1}) == 1
    assert detections_per_image_setting({"detections_per_image": 1000}) == 1000
    for bad in (0, 1001, "many", 2.5, True, None, -3):
        with pytest.raises(ValueError, match=r"inference_settings\.detections_per_image"):
            detections_per_image_setting({"detections_per_image": bad})


def _write_config(root, global_inf, dataset_inf):
    (root / "datasets").mkdir()
    (root / "config.yaml").write_text(yaml.safe_dump({"paths": {}, "inference_settings": global_inf}))
    if dataset_inf is not None:
        (root / "datasets" / "ds.yaml").write_text(yaml.safe_dump({"inference_overrides": dataset_inf}))


@pytest.mark.parametrize("global_inf,dataset_inf,want", [({}, None, 100), ({"detections_per_image": 300}, None, 300),
                                                         ({"detections_per_image": 300}, {"confidence_mode": "auto"}, 300),
                                                         ({"detections_per_image": 300}, {"detections_per_image": 640}, 640),
                                                         ({}, {"detections_per_image": 256}, 256)])
def test_dataset_file_overrides_the_global_file(tmp_path, monkeypatch, global_inf, dataset_inf, want):
    from deepemia_amd.functions.inference import PipelineSettings, detections_per_image_setting
    from deepemia_amd.utils import config as C

    _write_config(tmp_path, global_inf, dataset_inf)
    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(tmp_path))
    C.reset_cache()
    try:
        assert detections_per_image_setting(C.get_config(dataset_name="ds").get("inference_settings", {})) == want
        assert PipelineSettings("ds").detections_per_image == want          # what run_inference and the evaluate task read
    finally:
        C.reset_cache()


def test_a_bad_value_in_the_dataset_file_ends_the_run_before_any_model_is_loaded(tmp_path, monkeypatch):
    from deepemia_amd.functions.inference import PipelineSettings
    from deepemia_amd.utils import config as C

    _write_config(tmp_path, {}, {"detections_per_image": 1001})
    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(tmp_path))
    C.reset_cache()
    try:
        with pytest.raises(ValueError, match=r"inference_settings\.detections_per_image"):
            PipelineSettings("ds")
    finally:
        C.reset_cache()


def test_cfg_carries_the_value():
    from deepemia_amd.data.models import _cfg

    assert _cfg(50, 0.3, 2, "w.pth").TEST.DETECTIONS_PER_IMAGE == 100
    cfg = _cfg(101, 0.3, 2, "w.pth", 640)
    assert cfg.TEST.DETECTIONS_PER_IMAGE == 640
    assert (cfg.MODEL.DEPTH, cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST, cfg.MODEL.ROI_HEADS.NUM_CLASSES, cfg.MODEL.WEIGHTS) == (101, 0.3, 2, "w.pth")


def test_engine_range_check_needs_no_device():
    import numpy as np

    from deepemia_amd.engine import DETS_PER_IMAGE, MAX_DETS_PER_IMAGE, MaskRCNNEngine, check_dets_per_image

    assert (DETS_PER_IMAGE, MAX_DETS_PER_IMAGE) == (100, 1000)
    assert check_dets_per_image(1) == 1 and check_dets_per_image(1000) == 1000 and check_dets_per_image(np.int64(256)) == 256
    for bad in (0, 1001, -1, "many", 2.5, True, None):
        with pytest.raises(ValueError, match="dets_per_image"):
            check_dets_per_image(bad)
    # the constructor checks it before it looks for a device or a library
    with pytest.raises(ValueError, match="dets_per_image"):
        MaskRCNNEngine({}, 50, 2, 0.3, dets_per_image=1001)
