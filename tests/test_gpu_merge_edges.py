"""The tile-merge kernels at edge geometry, through the C ABI the way ``maskset.py`` and ``cropset.py`` call it, against the
independent dense references of ``merge_ref.py`` on the tables of ``merge_cases.py`` (``test_cpu_merge_ref.py`` checks both
without a GPU):

  * ``demia_mask_place_tiles`` (``place_tile_kernel``) and ``demia_crop_place_tiles`` (``crop_place_kernel``), which share
    ``mwords::placed_word``: the float64 nearest rule at sizes where the integer rule, the direct ratio and the float32 form
    each give another pixel; source widths that are no multiple of 32 with the padding bits of the source SET; offsets that
    are not word-aligned, negative, over the frame's edges and outside it; frames with a partly used last word;
  * ``demia_mask_overlap_prefix``: segments of more than 256 masks (the box kernel's second and third chunk of earlier masks),
    a segment that starts inside a chunk, pixels whose only earlier owner is 256, 257, 512 or 513 masks back (dense blobs
    alone would hide a kernel that stops after its first chunk: some nearer mask owns the pixel too), boxes tight, grown and
    absent;
  * ``demia_mask_column_counts``: frames wider than one 256-thread block, segment rows, box edges, the last column.

Everything is exact: bits and integers, no tolerance.  The test owns every destination: it holds ``SENTINEL`` before the call
where the kernel has to write every word, and ``GUARD`` words behind it that no kernel may touch.
"""
import numpy as np
import pytest
import torch

import merge_cases as T
import merge_ref as REF

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
GUARD = 1024


@pytest.fixture(scope="module")
def gpu(gpu_device):
    from deepemia_amd import _lib

    return dict(dev=gpu_device, lib=_lib.load(), L=_lib)


def _stream(g) -> int:
    return int(torch.cuda.current_stream(g["dev"]).cuda_stream)


def _dev(g, arr, dtype=np.int32):
    """Host array -> device tensor (None stays None); uint32 words travel as int32."""
    if arr is None:
        return None
    a = np.ascontiguousarray(arr)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    else:
        a = a.astype(dtype)
    return torch.from_numpy(a).to(g["dev"])


def _guarded(g, n: int, fill: int) -> torch.Tensor:
    """n words of ``fill`` and GUARD words of the sentinel behind them."""
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=g["dev"])
    buf[:n] = fill
    return buf


def _read(buf: torch.Tensor, n: int, what) -> np.ndarray:
    torch.cuda.synchronize()
    host = buf.cpu().numpy().view(np.uint32)
    assert host.shape == (n + GUARD,) and (host[n:] == SENTINEL).all(), (what, "the guard behind the buffer was written")
    return host[:n]


def _with_guard(g, words: np.ndarray) -> torch.Tensor:
    """Input / output planes on the device with the guard behind them."""
    flat = np.ascontiguousarray(words).reshape(-1)
    buf = _guarded(g, flat.size, 0)
    if flat.size:
        buf[:flat.size] = _dev(g, flat)
    return buf


# ------------------------------------------------------------------------------------------------------------------
# placement
# ------------------------------------------------------------------------------------------------------------------
PLACE_NAMES = [c.name for c in T.PLACE_CASES]


def _place_planes(g, c) -> np.ndarray:
    L, (H, W) = g["L"], c.frame
    wpr = (W + 31) // 32
    src = _dev(g, T.packed_sources(c))
    assert tuple(src.shape) == (c.T, c.src[0], (c.src[1] + 31) // 32)
    xo, yo = _dev(g, np.array(c.xo, dtype=np.int32)), _dev(g, np.array(c.yo, dtype=np.int32))
    n = c.T * H * wpr
    dst = _guarded(g, n, SENTINEL)
    L.check(g["lib"].demia_mask_place_tiles(L.ptr(src), L.ptr(dst), L.ptr(xo), L.ptr(yo), c.T, c.src[0], c.src[1], c.tile[0], c.tile[1],
                                            H, W, _stream(g)), "demia_mask_place_tiles")
    return _read(dst, n, c.name).reshape(c.T, H, wpr)


@pytest.mark.parametrize("name", PLACE_NAMES)
def test_place_tiles_planes(gpu, name):
    c = T.PLACE_BY_NAME[name]
    words = _place_planes(gpu, c)
    assert not (words == SENTINEL).any(), (name, "a destination word was not written")
    dense, pad = REF.unpack(words, c.frame[1])
    assert not pad.any(), (name, int(pad.sum()), "bits set at x >= W")
    want = T.placed(c)
    bad = np.argwhere(dense != want)
    assert bad.shape[0] == 0, (name, c.src, c.tile, bad.shape[0], "first (tile, y, x):", bad[:5].tolist(),
                               [c.offsets[t] for t in sorted({int(b[0]) for b in bad[:5]})])


def _room_layout(rooms: np.ndarray):
    """(exclusive prefix sums of rows x word columns per room, total): the layout of ``demia_mask_crop_pack``."""
    lens = np.array([0 if r[0] < 0 else (r[2] - r[0] + 1) * ((r[3] >> 5) - (r[1] >> 5) + 1) for r in rooms.tolist()], dtype=np.int64)
    offs = np.zeros(len(lens), dtype=np.int64)
    if len(lens):
        offs[1:] = np.cumsum(lens)[:-1]
    return offs, lens, int(lens.sum())


@pytest.mark.parametrize("loose", [False, True], ids=["rooms_of_placed_tiles", "rooms_grown"])
@pytest.mark.parametrize("name", PLACE_NAMES)
def test_place_tiles_crops(gpu, name, loose):
    from deepemia_amd.cropset import rooms_of_placed_tiles

    g, L, c = gpu, gpu["L"], T.PLACE_BY_NAME[name]
    H, W = c.frame
    rooms = rooms_of_placed_tiles(T.source_boxes(c), c.src, c.tile, c.xo, c.yo, c.frame)
    if loose:
        rooms = T.grow_boxes(rooms, c.frame, by=(3, 33, 2, 40))
    offs, lens, total = _room_layout(rooms)
    src = _dev(g, T.packed_sources(c))
    xo, yo = _dev(g, np.array(c.xo, dtype=np.int32)), _dev(g, np.array(c.yo, dtype=np.int32))
    room_d, offs_d = _dev(g, rooms.reshape(-1, 4)), _dev(g, offs, np.int64)
    payload = _guarded(g, total, SENTINEL)
    area = torch.full((c.T,), -5, dtype=torch.int32, device=g["dev"])
    bbox = torch.full((c.T, 4), -5, dtype=torch.int32, device=g["dev"])
    L.check(g["lib"].demia_crop_place_tiles(L.ptr(src), L.ptr(xo), L.ptr(yo), c.T, c.src[0], c.src[1], c.tile[0], c.tile[1], H, W,
                                            L.ptr(room_d), L.ptr(offs_d), L.ptr(payload), L.ptr(area), L.ptr(bbox), _stream(g)),
            "demia_crop_place_tiles")
    got = _read(payload, total, name)                 # (the guard starts at the last room's last word + 1)
    area_h, bbox_h = area.cpu().numpy(), bbox.cpu().numpy()
    want = T.placed(c)
    want_words = REF.pack(want, W)
    for m in range(c.T):
        what = (name, m, c.kinds[m], c.offsets[m], rooms[m].tolist())
        a, b = REF.area_bbox(want[m])
        assert int(area_h[m]) == a and bbox_h[m].tolist() == b, (what, int(area_h[m]), bbox_h[m].tolist(), a, b)
        if rooms[m, 0] < 0:
            assert a == 0 and lens[m] == 0, what         # nothing to write: the neighbours' words and the guard say it wrote nothing
            continue
        y0, x0, y1, x1 = rooms[m].tolist()
        ref = want_words[m, y0:y1 + 1, x0 >> 5:(x1 >> 5) + 1]
        # room m's words, and only they: its last word and room m + 1's first word are neighbours in the payload
        mine = got[offs[m]:offs[m] + lens[m]].reshape(ref.shape)
        assert np.array_equal(mine, ref), (what, int((mine != ref).sum()), "words differ; unwritten:", int((mine == SENTINEL).sum()))


@pytest.mark.parametrize("name", PLACE_NAMES)
def test_place_tiles_through_the_wrappers(gpu, name):
    """``MaskOps.place_tiles`` and ``CropMaskSet.place_tiles(...).to_planes()`` pass ``src_w`` and the offsets as the ABI expects."""
    from deepemia_amd.cropset import CropMaskSet, rooms_of_placed_tiles
    from deepemia_amd.maskset import MaskOps

    c = T.PLACE_BY_NAME[name]
    H, W = c.frame
    ops = MaskOps(gpu["dev"])
    src = _dev(gpu, T.packed_sources(c)).contiguous()
    want = REF.pack(T.placed(c), W)
    planes = ops.place_tiles(src, c.xo, c.yo, c.tile[0], c.tile[1], H, W, src_w=c.src[1])
    assert tuple(planes.shape) == want.shape
    assert np.array_equal(planes.cpu().numpy().view(np.uint32), want), name
    rooms = rooms_of_placed_tiles(T.source_boxes(c), c.src, c.tile, c.xo, c.yo, c.frame)
    cs = CropMaskSet.place_tiles(ops, src, rooms, c.xo, c.yo, c.tile[0], c.tile[1], H, W, src_w=c.src[1])
    back = cs.to_planes()
    assert tuple(back.shape) == want.shape
    assert np.array_equal(back.cpu().numpy().view(np.uint32), want), name
    assert np.array_equal(cs.area.cpu().numpy(), np.array([REF.area_bbox(m)[0] for m in T.placed(c)], dtype=np.int32))


# ------------------------------------------------------------------------------------------------------------------
# overlap removal
# ------------------------------------------------------------------------------------------------------------------
def _overlap(g, c, boxes) -> np.ndarray:
    """One ``demia_mask_overlap_prefix`` call on a fresh copy of the case's masks; returns the words [M, H, wpr]."""
    L, (H, W) = g["L"], c.frame
    words = REF.pack(T.overlap_masks(c), W)
    buf = _with_guard(g, words)
    seg, bb = _dev(g, c.seg()), _dev(g, boxes)
    L.check(g["lib"].demia_mask_overlap_prefix(L.ptr(buf), L.ptr(seg), L.ptr(bb), c.M, H, W, _stream(g)), "demia_mask_overlap_prefix")
    return _read(buf, words.size, c.name).reshape(words.shape)


@pytest.mark.parametrize("mode", T.BOX_MODES)
@pytest.mark.parametrize("name", [c.name for c in T.OVERLAP_CASES])
def test_overlap_prefix(gpu, name, mode):
    c = T.OVERLAP_BY_NAME[name]
    W = c.frame[1]
    want = REF.pack(T.overlap_want(c), W)                 # (padding bits 0: the result has to keep them 0)
    got = _overlap(gpu, c, T.overlap_boxes(c, mode))
    bad = np.unique(np.argwhere(got != want)[:, 0])
    assert bad.size == 0, (name, mode, f"{bad.size} of {c.M} masks differ from the reference, first:", bad[:8].tolist(),
                           "segment starts:", c.starts().tolist())
    if mode != "none":
        # the box kernel's workgroups race on purpose: the answer may not depend on their order, and is the streaming kernel's
        again = _overlap(gpu, c, T.overlap_boxes(c, mode))
        assert np.array_equal(again, got), (name, mode, "two runs on the same input differ")
        assert np.array_equal(_overlap(gpu, c, None), got), (name, mode, "box kernel and streaming kernel differ")


# ------------------------------------------------------------------------------------------------------------------
# column counts
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in T.COUNT_CASES])
def test_column_counts(gpu, name):
    g, L, c = gpu, gpu["L"], T.COUNT_BY_NAME[name]
    H, W = c.frame
    masks, seg = T.count_inputs(c)
    words = _dev(g, REF.pack(masks, W))
    seg_d, box_d = _dev(g, seg), _dev(g, T.count_boxes(c))          # (held until the kernel has run)
    assert seg is None or (len(seg) == len(masks) and int(seg.max()) < c.n_seg)
    counts = _guarded(g, c.n_seg * W, 0)                  # (the caller zeroes the counts)
    L.check(g["lib"].demia_mask_column_counts(L.ptr(words), L.ptr(seg_d), L.ptr(box_d), len(masks), H, W, L.ptr(counts), _stream(g)),
            "demia_mask_column_counts")
    got = _read(counts, c.n_seg * W, name).view(np.int32).reshape(c.n_seg, W).astype(np.int64)
    want = REF.column_counts(masks, seg, c.n_seg)
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, (name, bad.shape[0], "first (segment, column, got, want):",
                               [(int(s), int(x), int(got[s, x]), int(want[s, x])) for s, x in bad[:6]])
    for min_size in T.MIN_SIZES:                          # what the class pass derives: columns whose count is > min_size
        assert np.array_equal((got > min_size).sum(axis=1), (want > min_size).sum(axis=1)), (name, min_size)
    if seg is not None:
        assert not got[2].any() and not got[5].any()      # ids that no mask has


def test_column_counts_refuses_more_masks_than_a_grid_has_rows(gpu):
    """M = 65536 is one more than gridDim.y allows: the library's own error, before any launch.  (The buffers are real and every
    box is -1, so the call would be harmless even if it did launch.)"""
    g, L = gpu, gpu["L"]
    M = 65536
    words = torch.zeros((M, 1, 1), dtype=torch.int32, device=g["dev"])
    bbox = torch.full((M, 4), -1, dtype=torch.int32, device=g["dev"])
    counts = torch.zeros((32,), dtype=torch.int32, device=g["dev"])
    with pytest.raises(L.HipKernelError, match="65535"):
        L.check(g["lib"].demia_mask_column_counts(L.ptr(words), 0, L.ptr(bbox), M, 1, 32, L.ptr(counts), _stream(g)), "demia_mask_column_counts")
    torch.cuda.synchronize()
    assert not counts.any()
    # one fewer is served
    L.check(g["lib"].demia_mask_column_counts(L.ptr(words), 0, L.ptr(bbox), M - 1, 1, 32, L.ptr(counts), _stream(g)), "demia_mask_column_counts")
    torch.cuda.synchronize()
    assert not counts.any()
