"""Host side of crop-framed masks across ranks: the ``rank_exchange`` setting, the refusals that stay and the one that goes, and
the room / offset arithmetic ``CropMaskSet.from_table`` does on a gathered header."""
import types

import numpy as np
import pytest


def test_rank_exchange_defaults_to_planes_and_knows_two_values():
    from deepemia_amd.functions.inference import rank_exchange_setting
    assert rank_exchange_setting({}) == "planes" and rank_exchange_setting(None) == "planes"
    assert rank_exchange_setting({"rank_exchange": "planes", "mask_frame": "full"}) == "planes"
    assert rank_exchange_setting({"rank_exchange": "planes", "mask_frame": "crop"}) == "planes"
    for frame in ("crop", "crop_direct"):
        assert rank_exchange_setting({"rank_exchange": "crops", "mask_frame": frame}) == "crops"


def test_unknown_rank_exchange_names_both_values():
    from deepemia_amd.functions.inference import rank_exchange_setting
    with pytest.raises(ValueError) as e:
        rank_exchange_setting({"rank_exchange": "rooms", "mask_frame": "crop"})
    assert all(repr(v) in str(e.value) for v in ("planes", "crops")) and "'rooms'" in str(e.value)


@pytest.mark.parametrize("settings", [{"rank_exchange": "crops"}, {"rank_exchange": "crops", "mask_frame": "full"}])
def test_crops_with_the_full_frame_is_a_configuration_error(settings):
    from deepemia_amd.functions.inference import InferencePipeline, rank_exchange_setting
    with pytest.raises(ValueError, match="mask_frame"):
        rank_exchange_setting(settings)
    fake = types.SimpleNamespace(engine=types.SimpleNamespace(device="cpu"))
    with pytest.raises(ValueError, match="rank_exchange: crops"):
        InferencePipeline([fake], "t", settings, {})


@pytest.mark.parametrize("extra, word", [({"merge_mode": "soft_nms"}, "soft_nms"), ({"multiscale_settings": {"enabled": True}}, "multiscale")])
def test_the_modes_that_stay_on_full_are_still_refused_with_the_key(extra, word):
    from deepemia_amd.functions.inference import rank_exchange_setting
    with pytest.raises(ValueError, match=word):
        rank_exchange_setting(dict({"mask_frame": "crop_direct", "rank_exchange": "crops"}, **extra))


def _two_ranks(monkeypatch):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda: 1)
    monkeypatch.setattr(dist, "get_world_size", lambda: 2)


@pytest.mark.parametrize("frame", ["crop", "crop_direct"])
def test_crop_frames_at_two_ranks_need_the_key_and_the_refusal_names_it(monkeypatch, frame):
    from deepemia_amd.functions.inference import InferencePipeline
    fake = types.SimpleNamespace(engine=types.SimpleNamespace(device="cpu"))
    _two_ranks(monkeypatch)
    for settings in ({"mask_frame": frame}, {"mask_frame": frame, "rank_exchange": "planes"}):
        with pytest.raises(ValueError, match="one process only") as e:
            InferencePipeline([fake], "t", settings, {})
        assert "rank_exchange: crops" in str(e.value) and "use mask_frame: full" in str(e.value) and frame in str(e.value)
    pipe = InferencePipeline([fake], "t", {"mask_frame": frame, "rank_exchange": "crops"}, {})
    assert (pipe.world, pipe.rank, pipe.mask_frame, pipe.rank_exchange, pipe.crop) == (2, 1, frame, "crops", True)
    assert InferencePipeline([fake], "t", {"mask_frame": "full"}, {}).rank_exchange == "planes"


def test_table_layout_equals_the_instance_tables_own_arithmetic():
    """A header as an exchange returns it -- a marker row (unit -1, box -1), empty masks (box -1), boxes that start and end on word
    boundaries, one that fills a 300 x 417 frame -- back to back and at the positions of a gathered buffer."""
    from deepemia_amd import parallel
    from deepemia_amd.cropset import CropMaskSet, room_lengths
    boxes = np.array([[-1, -1, -1, -1], [5, 7, 5, 7], [0, 32, 9, 63], [-1, -1, -1, -1], [3, 30, 40, 97], [0, 0, 299, 416], [299, 416, 299, 416],
                      [-1, -1, -1, -1]], dtype=np.int32)
    hdr = np.zeros((len(boxes), parallel.HDR), dtype=np.int32)
    hdr[:, 0] = [-1, 0, 0, 1, 1, 2, 2, 3]
    hdr[:, 1] = [1, 0, 0, 0, 1, 1, 0, 0]
    hdr[:, 4:8] = boxes
    want_len = parallel._payload_lengths(hdr)
    assert want_len.tolist() == [0, 1, 10, 0, 38 * 4, 300 * 14, 1, 0]
    rows, off, lens = CropMaskSet.table_layout(hdr)
    assert np.array_equal(rows, np.arange(len(boxes))) and np.array_equal(lens, want_len) and np.array_equal(lens, room_lengths(boxes))
    assert np.array_equal(off, parallel._offsets(want_len)) and off.dtype == np.int64 and lens.dtype == np.int64
    # a gathered buffer: the words stay where the ranks put them, and the rows are picked class-major
    gathered = parallel._offsets(want_len)[::-1].copy() + 1000
    pick = np.array([6, 1, 2, 4, 5])
    rows, off, lens = CropMaskSet.table_layout(hdr, offsets=gathered, rows=pick)
    assert np.array_equal(rows, pick) and rows.dtype == np.int64 and np.array_equal(off, gathered) and np.array_equal(lens, want_len)
    with pytest.raises(AssertionError):
        CropMaskSet.table_layout(hdr, offsets=gathered[:-1])
