"""GPU tests of the outline-agreement kernels (``demia_mask_outline_agreement`` / ``demia_crop_outline_agreement``): every case of
``outline_cases`` on planes and on crop sets built from the same masks (rooms of the two sets grown differently, so they start
at different rows and word columns) equals the dense reference integer for integer -- ``n``, ``max_d2``, ``sum_d2``, ``sum_q``
and the histogram, in both directions; the same records come out of both frames, out of any number of workgroups, and the pair
list's edge sizes launch nothing."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import outline_cases as OC  # noqa: E402
import outline_ref as OR  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("n", "max_d2", "sum_d2", "sum_q", "hist")


@pytest.fixture(scope="module")
def ops():
    from deepemia_amd.maskset import MaskOps
    return MaskOps("cuda:0")


@pytest.fixture(scope="module")
def sizes(ops):
    """The LDS tile and the workgroup's share, as the library states them: a retuned kernel keeps its checkerboard case."""
    tile, share = int(ops.lib.demia_outline_target_tile()), int(ops.lib.demia_outline_source_share())
    assert tile >= 4 and share >= 1
    return tile, share


@pytest.fixture(scope="module")
def table(sizes):
    """The cases and their reference records, computed once."""
    return {name: (det, gt, pairs, OR.records(det, gt, pairs)) for name, det, gt, pairs in OC.cases(*sizes)}


NAMES = [c[0] for c in OC.cases()]


def _planes(ops, dense):
    M, H, W = dense.shape
    ops.set_frame_width(W)
    if M == 0:
        z = torch.zeros((0, H, (W + 31) // 32), dtype=torch.int32, device=ops.device)
        return z, torch.zeros((0, 4), dtype=torch.int32, device=ops.device), np.zeros(0, np.int64)
    planes = ops.from_dense(dense)
    area, bbox = ops.area_bbox(planes)
    return planes, bbox, area.cpu().numpy().astype(np.int64)


def _crop_set(ops, dense, seed):
    """The masks as a crop set whose rooms are the tight boxes grown by up to 40 pixels a side, differently per ``seed``."""
    from deepemia_amd.cropset import CropMaskSet

    M, H, W = dense.shape
    if M == 0:
        return CropMaskSet.empty(ops, (H, W))
    planes, bbox, _ = _planes(ops, dense)
    room = bbox.cpu().numpy().copy()
    g = np.random.RandomState(seed).randint(0, 41, room.shape)
    ok = room[:, 0] >= 0
    room[:, 0] = np.maximum(0, room[:, 0] - g[:, 0])
    room[:, 1] = np.maximum(0, room[:, 1] - g[:, 1])
    room[:, 2] = np.minimum(H - 1, room[:, 2] + g[:, 2])
    room[:, 3] = np.minimum(W - 1, room[:, 3] + g[:, 3])
    room[~ok] = -1
    return CropMaskSet.from_planes(ops, planes, W).reroom(room)


def _on_planes(ops, det, gt, pairs):
    from deepemia_amd.maskset import OutlineAgreement

    d, d_bbox, d_area = _planes(ops, det)
    g, g_bbox, g_area = _planes(ops, gt)
    res = ops.outline_agreement(d, d_bbox, d_area, g, g_bbox, g_area, pairs, W=det.shape[2])
    assert tuple(res.records.shape) == (len(pairs), 2, 136) and res.records.dtype == torch.int32
    return OutlineAgreement.from_host(res.records.cpu().numpy())


def _on_crops(ops, det, gt, pairs):
    from deepemia_amd.maskset import OutlineAgreement

    d_set, g_set = _crop_set(ops, det, 1), _crop_set(ops, gt, 2)
    res = d_set.outline_agreement(g_set, pairs)
    return OutlineAgreement.from_host(res.records.cpu().numpy()), d_set, g_set


def _assert_equal(got, want, what):
    for k in KEYS:
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:5].tolist())


@pytest.mark.parametrize("name", NAMES)
def test_planes_equal_the_reference_integer_for_integer(ops, table, name):
    det, gt, pairs, want = table[name]
    _assert_equal(_on_planes(ops, det, gt, pairs), want, name)


@pytest.mark.parametrize("name", NAMES)
def test_crop_sets_equal_the_reference_and_the_planes(ops, table, name):
    det, gt, pairs, want = table[name]
    got, d_set, g_set = _on_crops(ops, det, gt, pairs)
    _assert_equal(got, want, name)
    _assert_equal(got, _on_planes(ops, det, gt, pairs), name)
    # the rooms of the two sets start at different word columns and, where the frame has the rows for it, at different rows
    d_room, g_room = d_set.room_h, g_set.room_h
    n = min(len(d_room), len(g_room))
    assert ((d_room[:n, 1] >> 5) != (g_room[:n, 1] >> 5)).any()
    if name == "frame_45x70":
        assert (d_room[:n, 0] != g_room[:n, 0]).any()


def test_cases_reach_the_paths_they_are_named_for(table, sizes):
    tile, share = sizes
    want = table["checkerboard"][3]
    assert (want["n"][0] > 2 * max(tile, share)).all() and (want["n"][0] % tile != 0).all()
    assert want["n"][1, 0] < share and want["n"][2, 1] < share          # a small source against a tiled target, and the reverse
    assert table["far_1x47000"][3]["max_d2"][0, 0] == 46999 ** 2 > 2 ** 31
    b = table["bins"][3]
    assert b["max_d2"][:, 0].tolist()[:4] == [126 * 126, 126 * 126 + 1, 127 * 127, 2]
    assert [int(np.argmax(h)) for h in b["hist"][:, 0]][:7] == [126, 127, 127, 2, 3, 5, 0]
    assert b["sum_q"][3, 0] == 362 and b["sum_q"][4, 0] == 768          # floor(256 sqrt 2); a perfect square is exact
    f = table["frame_45x70"][3]
    assert (f["max_d2"][2] == 0).all() and (f["sum_q"][2] == 0).all() and f["hist"][2, 0, 0] == f["n"][2, 0] > 0       # identical masks
    assert f["max_d2"][5, 0] != f["max_d2"][5, 1]                        # ring against disc: the directions differ
    assert f["n"][1, 0] == 2 * 45 + 2 * 70 - 4                           # the whole frame: its border is the frame's edge


class _OneChunk:
    """The library with a chunk table of ONE workgroup per pair-direction: every share beyond the first is strided over."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def demia_outline_chunks(self, d_area, D, g_area, G, pairs, P, chunk_off):
        import ctypes
        np.ctypeslib.as_array(ctypes.cast(chunk_off, ctypes.POINTER(ctypes.c_int64)), shape=(2 * P + 1,))[:] = np.arange(2 * P + 1)
        return 2 * P


def test_any_number_of_workgroups_gives_the_same_records(ops, table):
    from deepemia_amd.maskset import MaskOps

    det, gt, pairs, want = table["checkerboard"]
    one = MaskOps("cuda:0")
    one.lib = _OneChunk(ops.lib)
    _assert_equal(_on_planes(one, det, gt, pairs), want, "one workgroup per pair-direction")


def test_chunk_table_counts_pixels_per_share(ops, sizes):
    tile, share = sizes
    d_area = np.asarray([0, 1, share, share + 1, 300 * share], dtype=np.int64)
    g_area = np.asarray([3 * share - 1], dtype=np.int64)
    pairs = np.asarray([[0, 0], [1, 0], [2, 0], [3, 0], [4, 0]], dtype=np.int32)
    off = np.zeros(11, dtype=np.int64)
    total = ops.lib.demia_outline_chunks(d_area.ctypes.data, 5, g_area.ctypes.data, 1, pairs.ctypes.data, 5, off.ctypes.data)
    assert np.diff(off).tolist() == [1, 3, 1, 3, 1, 3, 2, 3, 256, 3] and total == off[-1]


@pytest.mark.parametrize("case", OC.edge_lists(), ids=lambda c: c[0])
def test_edge_sizes_of_the_pair_list_give_empty_records(ops, case):
    name, det, gt, pairs = case
    got = _on_planes(ops, det, gt, pairs)
    got_c, _, _ = _on_crops(ops, det, gt, pairs)
    for g in (got, got_c):
        assert all(g[k].shape[0] == 0 for k in KEYS)


def test_a_pair_outside_its_set_is_refused(ops, table):
    det, gt, _, _ = table["frame_45x70"]
    d, d_bbox, d_area = _planes(ops, det)
    g, g_bbox, g_area = _planes(ops, gt)
    for bad in ([[7, 0]], [[0, 7]], [[-1, 0]]):
        with pytest.raises(ValueError, match="outside its set"):
            ops.outline_agreement(d, d_bbox, d_area, g, g_bbox, g_area, np.asarray(bad), W=det.shape[2])
