"""Model discovery and loading kept as a drop-in (reference ``src/data/models.py:33-162``).

``choose_and_use_model`` returns ``(predictor, metadata)`` exactly like the reference, but the
predictor is the MI355X-native :class:`deepemia_amd.predictor.Predictor` instead of Detectron2's
``DefaultPredictor``.  The checkpoint is the Detectron2 file the reference writes / reads
(``<split_dir>/<dataset>/rcnn_r{50,101}/model_final_r{50,101}.pth``, ``torch.save({"model": sd})``).
There is no quantised / CPU fallback branch: without a HIP device loading fails loudly.
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import Dict, Tuple

import torch

from ..engine import MaskRCNNEngine
from ..predictor import Predictor
from ..utils.logger_utils import system_logger
from .datasets import MetadataCatalog

# BASELINE.json configs[1] runs bf16; parity (mask IoU >= 0.999 vs the fp32 CPU path) needs f32 arithmetic:
#   f16x2  f32 operands as two fp16 planes with exact power-of-two scales, three fp16 MFMAs per product, f32
#          accumulation (default: error <= 3 * 2^-22 per product, the same parity results as f32, ~1.8x faster)
#   f32x3  f32 operands split into three bf16 planes, six bf16 MFMAs per product (no operand scales needed)
#   f32    the exact-f32 MFMA (v_mfma_f32_32x32x2_f32)
#   bf16x2 / bf16   16-bit / 8-bit significand operands (faster still, mask IoU parity NOT met)
DEFAULT_PRECISION = os.environ.get("DEEPEMIA_PRECISION", "f16x2")
# INPUT.MIN_SIZE_TEST / MAX_SIZE_TEST: the reference never overrides the model-zoo 800 / 1333 (models.py:134-144), so
# these are the parity values.  DEEPEMIA_MIN_SIZE_TEST / DEEPEMIA_MAX_SIZE_TEST select the flagged NON-parity
# "native resolution" mode (e.g. 2048 / 2048: the net sees a 2048^2 tile unscaled; 5x the work per tile).
MIN_SIZE_TEST = int(os.environ.get("DEEPEMIA_MIN_SIZE_TEST", "800"))
MAX_SIZE_TEST = int(os.environ.get("DEEPEMIA_MAX_SIZE_TEST", "1333"))


def get_trained_model_paths(base_dir: str, rcnn: int = 101) -> dict:
    """``{dataset: path}`` of every ``<base_dir>/<dataset>/rcnn_r<rcnn>/model_final_r<rcnn>.pth``."""
    out = {}
    for dataset_name in os.listdir(base_dir):
        path = os.path.join(base_dir, dataset_name, f"rcnn_r{rcnn}", f"model_final_r{rcnn}.pth")
        if os.path.exists(path):
            out[dataset_name] = path
    return out


def _cfg(rcnn: int, threshold: float, num_classes: int, weights: str, detections_per_image: int = 100) -> SimpleNamespace:
    """The three overrides of ``models.py:140-144`` on top of mask_rcnn_R_<rcnn>_FPN_3x, and ``TEST.DETECTIONS_PER_IMAGE``
    (the model zoo's 100, which the reference never overrides, unless ``inference_settings.detections_per_image`` says otherwise)."""
    roi = SimpleNamespace(SCORE_THRESH_TEST=threshold, NUM_CLASSES=num_classes)
    model = SimpleNamespace(DEVICE="cuda", ROI_HEADS=roi, WEIGHTS=weights, DEPTH=rcnn)
    return SimpleNamespace(MODEL=model, TEST=SimpleNamespace(DETECTIONS_PER_IMAGE=detections_per_image))


def read_d2_checkpoint(path: str) -> Dict[str, torch.Tensor]:
    ck = torch.load(path, map_location="cpu", weights_only=False)
    sd = ck["model"] if isinstance(ck, dict) and "model" in ck else ck
    return {k: (v if isinstance(v, torch.Tensor) else torch.as_tensor(v)) for k, v in sd.items()}


def load_model(cfg, model_path: str, dataset_name: str, is_quantized: bool = False) -> Predictor:
    """``DefaultPredictor(cfg)`` replacement (``models.py:54-107``)."""
    if is_quantized:
        raise RuntimeError("Quantized model load failed.")  # the reference's caller falls back on this
    cfg.MODEL.WEIGHTS = model_path
    metadata = MetadataCatalog.get(f"{dataset_name}_train")
    cfg.MODEL.ROI_HEADS.NUM_CLASSES = len(metadata.thing_classes)
    sd = read_d2_checkpoint(model_path)
    device = f"cuda:{torch.cuda.current_device()}" if torch.cuda.is_available() else "cuda:0"
    dets = int(getattr(getattr(cfg, "TEST", None), "DETECTIONS_PER_IMAGE", 100))
    eng = MaskRCNNEngine(sd, cfg.MODEL.DEPTH, cfg.MODEL.ROI_HEADS.NUM_CLASSES, cfg.MODEL.ROI_HEADS.SCORE_THRESH_TEST,
                         device, DEFAULT_PRECISION, MIN_SIZE_TEST, MAX_SIZE_TEST, dets_per_image=dets)
    if dets != 100:
        system_logger.warning(f"TEST.DETECTIONS_PER_IMAGE = {dets}: not the reference's 100 -- results are NOT comparable with "
                              f"the reference's")
    if (MIN_SIZE_TEST, MAX_SIZE_TEST) != (800, 1333):
        system_logger.warning(f"INPUT.MIN_SIZE_TEST / MAX_SIZE_TEST = {MIN_SIZE_TEST} / {MAX_SIZE_TEST}: not the reference's "
                              f"800 / 1333 -- results are NOT comparable with the reference's")
    if eng.unmatched_keys:
        system_logger.warning(f"{model_path}: {len(eng.unmatched_keys)} checkpoint keys were not consumed: "
                              f"{eng.unmatched_keys[:8]}{' ...' if len(eng.unmatched_keys) > 8 else ''}")
    return Predictor(eng)


def choose_and_use_model(model_paths: dict, dataset_name: str, threshold: float, metadata, rcnn: int = 101
                         ) -> Tuple[Predictor, object]:
    """``(predictor, metadata)`` or ``(None, None)`` when the dataset has no model (``models.py:110-162``)."""
    if dataset_name not in model_paths:
        system_logger.error(f"No model found for dataset {dataset_name}")
        return None, None
    from ..functions.inference import detections_per_image_setting      # (that module imports this one)
    from ..utils.config import get_config
    dets = detections_per_image_setting(get_config(dataset_name=dataset_name).get("inference_settings", {}))
    cfg = _cfg(rcnn, threshold, len(metadata.thing_classes), model_paths[dataset_name], dets)
    system_logger.info(f"Using standard model for {dataset_name}")
    return load_model(cfg, model_paths[dataset_name], dataset_name, is_quantized=False), metadata
