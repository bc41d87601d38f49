"""GPU tests of the boundary-band kernel (``csrc/boundary.hip``): both entries bit for bit against the CPU statement of the band
(``boundary_ref``) on every case of ``boundary_cases``, one mask against the batch, crops in tight and grown rooms with poisoned
surroundings and canaries behind everything written, the source left alone, and the band cross matrix against the dense
boundary IoU."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import boundary_cases as BC  # noqa: E402
import boundary_ref as BR  # noqa: E402

pytestmark = pytest.mark.gpu

CANARY = -1                             # all ones: a canary, and the poison of everything a kernel must not read


@pytest.fixture(scope="module")
def ops():
    from deepemia_amd.maskset import MaskOps
    return MaskOps("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(H, W, d):
    """(names, dense masks, reference bands) of one frame and width, computed once and shared."""
    names, dense = BC.masks(H, W, d)
    bands = np.stack([BR.band(m, d) for m in dense])
    dense.setflags(write=False)
    bands.setflags(write=False)
    return names, dense, bands


def _planes(ops, dense, W):
    planes = ops.from_dense(dense)
    ops.set_frame_width(W)
    area, bbox = ops.area_bbox(planes)
    return planes, area, bbox


def _room_words(m, room):
    """The words of dense mask ``m`` as a room stores them (rows y0 .. y1 x word columns x0 >> 5 .. x1 >> 5), int32."""
    y0, x0, y1, x1 = (int(v) for v in room)
    if y0 < 0:
        return np.zeros((0,), np.int32)
    c0, c1 = x0 >> 5, x1 >> 5
    bits = np.zeros((y1 - y0 + 1, (c1 - c0 + 1) * 32), dtype=bool)
    sub = m[y0:y1 + 1, c0 * 32:(c1 + 1) * 32]
    bits[:, :sub.shape[1]] = sub
    return np.packbits(bits.reshape(bits.shape[0], -1, 32), axis=-1, bitorder="little").view("<u4").reshape(-1).view(np.int32)


# ---- both entries against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", BC.FRAMES)
def test_both_entries_equal_the_reference_band_bit_for_bit(ops, H, W):
    from deepemia_amd.cropset import CropMaskSet

    rng = np.random.RandomState(H + 7 * W)
    for d in BC.widths(H, W):
        names, dense, bands = _case(H, W, d)
        planes, area, bbox = _planes(ops, dense, W)
        keep = planes.clone()
        want, want_area = ops.from_dense(bands), torch.from_numpy(bands.reshape(len(bands), -1).sum(1).astype(np.int32)).to(ops.device)
        got, got_area = ops.boundary_band(planes, bbox, d, W)
        bad = [names[i] for i in range(len(names)) if not torch.equal(got[i], want[i])]
        assert not bad, (d, bad)
        assert torch.equal(got_area, want_area), d
        assert torch.equal(planes, keep)                                                   # the source is only read
        # the band is a subset of the mask with the mask's tight box
        _, band_bbox = ops.area_bbox(got)
        assert torch.equal(band_bbox, bbox) and not bool((got & ~planes).any())
        # crops: rooms that are the tight boxes, and rooms grown by up to 9 px
        tight = CropMaskSet.from_planes(ops, planes, W)
        grown = tight.reroom(BC.grown_rooms(rng, tight.room_h, H, W))
        for cset in (tight, grown):
            pay = cset.payload.clone()
            bset = cset.boundary_band(d)
            assert np.array_equal(bset.room_h, cset.room_h) and bset.offsets is cset.offsets and len(bset) == len(cset)
            assert torch.equal(bset.to_planes(), got), d
            assert torch.equal(bset.area, want_area) and torch.equal(bset.bbox, bbox)
            assert torch.equal(cset.payload, pay)
        # one mask alone gives what it gives in the batch
        for name in ("full", "square_with_hole", "blob_3", "pixel_last"):
            i = names.index(name)
            one, one_area = ops.boundary_band(planes[i:i + 1], bbox[i:i + 1], d, W)
            assert torch.equal(one[0], got[i]) and int(one_area[0]) == int(want_area[i]), (d, name)
            alone = tight.select([i]).boundary_band(d)
            assert torch.equal(alone.to_planes()[0], got[i]) and int(alone.area[0]) == int(want_area[i]), (d, name)


def test_a_width_below_one_is_refused(ops):
    from deepemia_amd import _lib
    from deepemia_amd.cropset import CropMaskSet

    planes, area, bbox = _planes(ops, np.ones((2, 5, 33), dtype=bool), 33)
    for d in (0, -1):
        with pytest.raises(ValueError, match="d must be an integer >= 1"):
            ops.boundary_band(planes, bbox, d, 33)
        with pytest.raises(ValueError, match="d must be an integer >= 1"):
            CropMaskSet.from_planes(ops, planes, 33).boundary_band(d)
    out, scratch, n = torch.zeros_like(planes), torch.zeros_like(planes), torch.zeros((2,), dtype=torch.int32, device=ops.device)
    st = ops.lib.demia_mask_boundary_band(_lib.ptr(planes), _lib.ptr(bbox), 2, 5, 33, 0, _lib.ptr(out), _lib.ptr(n), _lib.ptr(scratch), ops._stream())
    assert st != 0 and b"d" in ops.lib.demia_last_error()
    torch.cuda.synchronize()
    assert not bool(out.any())
    empty, empty_area = ops.boundary_band(planes[:0], bbox[:0], 3, 33)                       # M == 0: no launch
    assert empty.shape == (0, 5, 2) and empty_area.shape == (0,)
    assert len(CropMaskSet.empty(ops, (5, 33)).boundary_band(3)) == 0


# ---- crops with poisoned surroundings, canaries behind what is written -----------------------------------------------------------
@pytest.mark.parametrize("H,W", BC.FRAMES)
def test_crop_entry_reads_only_its_room_and_writes_only_its_box(ops, H, W):
    """Every mask sits in a room grown by up to 9 px, between two POISON entries -- rooms of all ones with an empty box, which the
    kernel must neither read for a neighbour nor write a band for -- and between gaps of all ones; the output payload is zero in
    the rooms and canaries in the gaps; the areas and the scratch end in canaries."""
    from deepemia_amd import _lib
    from deepemia_amd.cropset import room_lengths

    rng = np.random.RandomState(3 * H + W)
    for d in BC.widths(H, W):
        names, dense, bands = _case(H, W, d)
        n = len(dense)
        boxes = np.asarray([BR.tight_box(m) for m in dense], dtype=np.int32)
        rooms = np.full((2 * n + 1, 4), -1, dtype=np.int32)
        rooms[1::2] = BC.grown_rooms(rng, boxes, H, W)
        ph, pw = min(H, 3), min(W, 40)
        rooms[0::2] = [0, 0, ph - 1, pw - 1]                                                # the poison entries
        bbox_h = np.full((2 * n + 1, 4), -1, dtype=np.int32)
        bbox_h[1::2] = boxes
        M = len(rooms)
        lens = room_lengths(rooms)
        gap = 3
        off = (np.cumsum(lens + gap) - lens).astype(np.int64)
        total = int(off[-1] + lens[-1] + gap)
        src = np.full(total, CANARY, dtype=np.int32)
        out = np.full(total, CANARY, dtype=np.int32)
        want = out.copy()
        for k in range(n):
            m = 2 * k + 1
            src[off[m]:off[m] + lens[m]] = _room_words(dense[k], rooms[m])
            out[off[m]:off[m] + lens[m]] = 0
            want[off[m]:off[m] + lens[m]] = _room_words(bands[k], rooms[m])
        for m in range(0, M, 2):
            out[off[m]:off[m] + lens[m]] = 0                                              # (zero as the contract asks; must stay zero)
            want[off[m]:off[m] + lens[m]] = 0
        soff = np.zeros(M, dtype=np.int64)
        stotal = int(ops.lib.demia_crop_boundary_scratch(rooms.ctypes.data, M, H, W, soff.ctypes.data))
        assert stotal == int(lens[lens > BC.LARGE_WORDS].sum())
        if (H, W) == (640, 640):
            assert stotal >= 640 * 20                                                       # the frame-sized masks work in scratch
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)           # noqa: E731
        t_src, t_out, t_room, t_off, t_bbox, t_soff = dev(src), dev(out), dev(rooms), dev(off), dev(bbox_h), dev(soff)
        t_area = torch.full((M + 1,), CANARY, dtype=torch.int32, device=ops.device)
        t_scr = torch.full((stotal + 8,), CANARY, dtype=torch.int32, device=ops.device)
        _lib.check(ops.lib.demia_crop_boundary_band(_lib.ptr(t_src), _lib.ptr(t_room), _lib.ptr(t_off), _lib.ptr(t_bbox), M, H, W, d,
                                                    _lib.ptr(t_out), _lib.ptr(t_area), _lib.ptr(t_scr[4:]), _lib.ptr(t_soff), ops._stream()),
                   "demia_crop_boundary_band")
        got, area, scr = t_out.cpu().numpy(), t_area.cpu().numpy(), t_scr.cpu().numpy()
        for k in range(n):
            m = 2 * k + 1
            assert np.array_equal(got[off[m]:off[m] + lens[m]], want[off[m]:off[m] + lens[m]]), (d, names[k])
        assert np.array_equal(got, want), d                                                # gaps and poison rooms included
        assert area[M] == CANARY and (area[0:M:2] == 0).all()
        assert np.array_equal(area[1:M:2], bands.reshape(n, -1).sum(1)), d
        assert (scr[:4] == CANARY).all() and (scr[-4:] == CANARY).all()
        assert np.array_equal(t_src.cpu().numpy(), src)                                    # the source set is unchanged


def test_plane_entry_writes_only_the_boxes_and_its_areas(ops):
    """The plane entry with canaries: the output planes are handed over as all ones -- the kernel writes the words of each box and
    nothing else --, the areas end in a canary, and the scratch planes are only touched for regions beyond the LDS buffer."""
    from deepemia_amd import _lib

    for (H, W), d in (((70, 100), 3), ((640, 640), 58)):
        names, dense, bands = _case(H, W, d)
        pick = [names.index(n) for n in ("full", "pixel", "empty", "edge_right", "square_with_hole", "blob_5", "blob_6")]
        dense, bands = dense[pick], bands[pick]
        planes, _, bbox = _planes(ops, dense, W)
        M, wpr = len(pick), (W + 31) // 32
        out = torch.full_like(planes, CANARY)
        scratch = torch.full((M + 1, H, wpr), CANARY, dtype=torch.int32, device=ops.device)
        area = torch.full((M + 1,), CANARY, dtype=torch.int32, device=ops.device)
        _lib.check(ops.lib.demia_mask_boundary_band(_lib.ptr(planes), _lib.ptr(bbox), M, H, W, d, _lib.ptr(out), _lib.ptr(area), _lib.ptr(scratch),
                                                    ops._stream()), "demia_mask_boundary_band")
        want = ops.from_dense(bands).cpu().numpy()
        got, bb = out.cpu().numpy(), bbox.cpu().numpy()
        for i in range(M):
            exp = np.full((H, wpr), CANARY, dtype=np.int32)
            if bb[i, 0] >= 0:
                y0, x0, y1, x1 = bb[i]
                exp[y0:y1 + 1, x0 >> 5:(x1 >> 5) + 1] = want[i, y0:y1 + 1, x0 >> 5:(x1 >> 5) + 1]
            assert np.array_equal(got[i], exp), i
        a = area.cpu().numpy()
        assert a[M] == CANARY and np.array_equal(a[:M], bands.reshape(M, -1).sum(1))
        s = scratch.cpu().numpy()
        assert (s[M] == CANARY).all()
        large = [i for i in range(M) if bb[i, 0] >= 0 and (bb[i, 2] - bb[i, 0] + 1) * ((bb[i, 3] >> 5) - (bb[i, 1] >> 5) + 1) > BC.LARGE_WORDS]
        assert bool(large) == ((H, W) == (640, 640))
        for i in range(M):
            if i not in large:
                assert (s[i] == CANARY).all(), i


# ---- band counts -> boundary IoU --------------------------------------------------------------------------------------------------
def test_band_cross_matrix_gives_the_dense_boundary_iou(ops):
    from deepemia_amd import cocoeval as CE
    from deepemia_amd.cropset import CropMaskSet

    H, W, d = 70, 100, 3
    names, dense, bands = _case(H, W, d)
    blobs = [i for i, n in enumerate(names) if n.startswith("blob_")]
    di, gi = blobs[:24] + [names.index("full"), names.index("empty")], blobs[24:44] + [names.index("square_with_hole"), names.index("empty")]
    D, G = len(di), len(gi)
    crowd = (np.arange(G) % 5 == 0).astype(np.uint8)
    want = np.array([[BR.boundary_iou(dense[a], dense[g], d, bool(crowd[j])) for j, g in enumerate(gi)] for a in di])
    want_task = np.minimum(want, np.array([[BR.mask_iou(dense[a], dense[g], bool(crowd[j])) for j, g in enumerate(gi)] for a in di]))
    mask_only = np.array([[BR.mask_iou(dense[a], dense[g], bool(crowd[j])) for j, g in enumerate(gi)] for a in di])
    # the pairs do overlap, crowd columns included, and each of the two IoUs is the smaller one somewhere
    assert np.count_nonzero(want) > 10 * D and np.count_nonzero(want[:, crowd == 1]) > D
    assert (want_task < want).any() and (want_task < mask_only).any()
    d_planes, d_area, d_bbox = _planes(ops, dense[di], W)
    g_planes, g_area, g_bbox = _planes(ops, dense[gi], W)
    d_band, d_ba = ops.boundary_band(d_planes, d_bbox, d, W)
    g_band, g_ba = ops.boundary_band(g_planes, g_bbox, d, W)
    inter = CE.cross_matrix(ops, d_band, d_bbox, None, g_band, g_bbox, None, W).cpu().numpy()
    got = CE.boundary_iou(inter, d_ba.cpu().numpy(), g_ba.cpu().numpy(), crowd)
    assert np.array_equal(got, want)
    m_inter = CE.cross_matrix(ops, d_planes, d_bbox, None, g_planes, g_bbox, None, W).cpu().numpy()
    m_iou = CE.mask_iou(m_inter, d_area.cpu().numpy(), g_area.cpu().numpy(), crowd)
    assert np.array_equal(np.minimum(m_iou, got), want_task)
    # the same over rooms
    d_set, g_set = CropMaskSet.from_planes(ops, d_planes, W), CropMaskSet.from_planes(ops, g_planes, W)
    db, gb = d_set.boundary_band(d), g_set.boundary_band(d)
    inter_c = CE.cross_matrix_crop(ops, db, None, gb, None).cpu().numpy()
    assert np.array_equal(inter_c, inter)
    assert np.array_equal(CE.boundary_iou(inter_c, db.area.cpu().numpy(), gb.area.cpu().numpy(), crowd), want)
