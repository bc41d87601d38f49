"""Host side of ``mask_frame: crop_direct``: the setting, and ``demia_crop_contour_scratch`` (host code behind the C ABI: the scratch a
crop-framed contour trace needs, from the rooms alone) against a NumPy restatement of its rule."""
import numpy as np
import pytest

TRACE_WORDS = 8192          # the trace's large LDS buffer, in words (csrc/contours.hip)


# ----------------------------------------------------------------------------------------------------------------- scratch
def _restated_scratch(room, H, W):
    """Per mask: the region of its ROOM grown by one ring and clipped to the frame, rows x word columns; padded by one more row /
    word on every side; two such buffers when the padded region exceeds TRACE_WORDS, nothing otherwise."""
    room = np.asarray(room, dtype=np.int64).reshape(-1, 4)
    ry0, ry1 = np.maximum(room[:, 0] - 1, 0), np.minimum(room[:, 2] + 1, H - 1)
    wx0, wx1 = np.maximum(room[:, 1] - 1, 0) >> 5, np.minimum(room[:, 3] + 1, W - 1) >> 5
    pn = (ry1 - ry0 + 1 + 2) * (wx1 - wx0 + 1 + 2)
    lens = np.where((room[:, 0] >= 0) & (pn > TRACE_WORDS), 2 * pn, 0)
    return lens, pn


def _native_scratch(room, H, W):
    from deepemia_amd import _lib
    lib = _lib.load()
    room = np.ascontiguousarray(room, dtype=np.int32).reshape(-1, 4)
    off = np.full(max(len(room), 1), -7, dtype=np.int64)
    total = int(lib.demia_crop_contour_scratch(room.ctypes.data, len(room), H, W, off.ctypes.data))
    return off[:len(room)], total


def _check(room, H, W):
    off, total = _native_scratch(room, H, W)
    lens, pn = _restated_scratch(room, H, W)
    assert np.array_equal(off, np.concatenate(([0], np.cumsum(lens)[:-1]))[:len(lens)])      # exclusive prefix sums
    assert total == int(lens.sum())
    assert np.all(lens[pn <= TRACE_WORDS] == 0)
    return lens, pn


def test_scratch_of_random_rooms_equals_the_restated_rule():
    H, W = 700, 4000                                                             # 125 words per row, W no multiple of 32
    g = np.random.default_rng(3)
    n = 400
    y0, x0 = g.integers(0, H, n), g.integers(0, W, n)
    y1 = np.minimum(y0 + g.integers(0, H, n), H - 1)
    x1 = np.minimum(x0 + g.integers(0, W, n), W - 1)
    room = np.stack([y0, x0, y1, x1], axis=1)
    room[g.random(n) < 0.1] = -1                                                 # empty rooms
    fixed = [[0, 0, 40, 3000], [H - 300, 10, H - 1, 2000], [5, 0, 600, 900], [3, W - 1200, 500, W - 1],      # the four frame edges
             [0, 0, H - 1, W - 1],                                               # the whole frame
             [-1, -1, -1, -1], [0, 0, 0, 0], [H - 1, W - 1, H - 1, W - 1]]
    room = np.concatenate([room, np.asarray(fixed)])
    lens, pn = _check(room, H, W)
    assert (lens > 0).sum() > 50 and (lens[room[:, 0] >= 0] == 0).sum() > 50     # both kinds occur
    assert lens[-4] == 2 * (H + 2) * ((W + 31) // 32 + 2)                        # whole frame: rows and word columns of the frame, padded
    assert _native_scratch(np.zeros((0, 4), np.int32), H, W)[1] == 0


def test_scratch_is_zero_at_the_limit_and_two_regions_one_row_above_it():
    H, W = 320, 1000
    # rows 10 .. 261 -> region rows 9 .. 262 = 254, padded 256; columns 64 .. 959 -> region words 1 .. 30 = 30, padded 32: 8192 words
    at = [10, 64, 261, 959]
    above = [10, 64, 262, 959]                                                   # one more row: 257 x 32 = 8224
    lens, pn = _check(np.asarray([at, above, at]), H, W)
    assert pn.tolist() == [8192, 8224, 8192] and lens.tolist() == [0, 2 * 8224, 0]
    # the same room flush with the frame's top: the ring row is clipped away, the region is one row smaller
    lens, pn = _check(np.asarray([[0, 64, 252, 959], [0, 64, 253, 959]]), H, W)
    assert pn.tolist() == [8192, 8224] and lens.tolist() == [0, 2 * 8224]


# ----------------------------------------------------------------------------------------------------------------- setting
def test_mask_frame_accepts_crop_direct():
    from deepemia_amd.functions.inference import MASK_FRAMES, mask_frame_setting
    assert MASK_FRAMES == ("full", "crop", "crop_direct")
    assert mask_frame_setting({"mask_frame": "crop_direct"}) == "crop_direct"
    assert mask_frame_setting({}) == "full"                                      # the default stays


@pytest.mark.parametrize("extra, word", [({"merge_mode": "soft_nms"}, "soft_nms"), ({"multiscale_settings": {"enabled": True}}, "multiscale")])
def test_crop_direct_with_the_modes_that_stay_on_full_is_refused(extra, word):
    from deepemia_amd.functions.inference import mask_frame_setting
    with pytest.raises(ValueError, match=word) as e:
        mask_frame_setting(dict({"mask_frame": "crop_direct"}, **extra))
    assert "crop_direct" in str(e.value)


def test_unknown_mask_frame_names_the_three_values():
    from deepemia_amd.functions.inference import mask_frame_setting
    with pytest.raises(ValueError) as e:
        mask_frame_setting({"mask_frame": "direct"})
    assert all(repr(v) in str(e.value) for v in ("full", "crop", "crop_direct")) and "'direct'" in str(e.value)


def test_pipeline_crop_is_true_for_both_crop_frames_and_ranks_are_refused(monkeypatch):
    import types
    import torch.distributed as dist
    from deepemia_amd.functions.inference import InferencePipeline
    fake = types.SimpleNamespace(engine=types.SimpleNamespace(device="cpu"))
    flags = {f: (p.crop, p.crop_direct) for f in ("full", "crop", "crop_direct") for p in [InferencePipeline([fake], "t", {"mask_frame": f}, {})]}
    assert flags == {"full": (False, False), "crop": (True, False), "crop_direct": (True, True)}
    pipe = InferencePipeline([fake], "t", {"mask_frame": "crop_direct"}, {})
    pipe.begin_image_stats()
    assert pipe.end_image_stats((8, 8)) == {"mask_frame": "crop_direct", "full_frame_planes_peak": 0, "plane_pool_capacity": 0}
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_rank", lambda: 1)
    monkeypatch.setattr(dist, "get_world_size", lambda: 2)
    for f in ("crop", "crop_direct"):
        with pytest.raises(ValueError, match="one process only"):
            InferencePipeline([fake], "t", {"mask_frame": f}, {})
