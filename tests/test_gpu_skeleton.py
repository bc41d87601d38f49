"""``demia_mask_skeleton`` / ``demia_crop_skeleton`` -- the morphological skeleton of a mask and, per contour, its length, end and
branch points -- against the literal reference of ``tests/skeleton_ref.py`` on the masks of ``tests/skeleton_cases.py``, traced by
the product's own tracer: the skeleton itself bit for bit (``skel_out``), the six integers equal, the two derived values within
4 ulp; then position and layout invariance, the crop entry against the plane entry, the scratch contract, ``ContourSet`` and the CLI."""
import csv
import io

import numpy as np
import pytest

import skeleton_cases as SC
import skeleton_ref as SR
from test_gpu_inscribed import _crop_scratch, _crop_tables, _frame_of_cases, _spy_copies, _trace

pytestmark = pytest.mark.gpu

UM = 0.37
COLS = SR.SKELETON_COLS
OUT_FILL = -7.25
OUT_GUARD = 6 * COLS
CANARY = 0x5A5A5A5A
LARGE_WORDS = 8192                                                       # the tracer's large LDS buffer (words per region buffer)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _pack(mask):
    """[H, W] bool -> [H, ceil(W / 32)] uint32, bit (x & 31) of word (x >> 5)."""
    H, W = mask.shape
    wpr = (W + 31) // 32
    m = np.zeros((H, wpr * 32), dtype=bool)
    m[:, :W] = mask
    return np.packbits(m.reshape(H, wpr, 32), axis=-1, bitorder="little").view(np.uint32).reshape(H, wpr)


def _region(box, H, W):
    """(ry0, ry1, wx0, wx1), inclusive: the box grown by one ring, clipped to the frame, in rows and word columns."""
    y0, x0, y1, x1 = (int(v) for v in box)
    return max(y0 - 1, 0), min(y1 + 1, H - 1), max(x0 - 1, 0) >> 5, min(x1 + 1, W - 1) >> 5


@pytest.fixture(scope="module")
def ops(gpu_device):
    from deepemia_amd.maskset import MaskOps
    return MaskOps(gpu_device)


@pytest.fixture(scope="module")
def cases():
    return SC.by_name()


@pytest.fixture(scope="module")
def refs(cases):
    """name -> Reference (skeleton and components), computed once and shared."""
    return {name: SR.Reference(c.mask) for name, c in cases.items()}


def _canary(dev, n, guard=0):
    import torch
    return torch.from_numpy(np.full(n + guard, CANARY, dtype=np.uint32).view(np.int32)).to(dev)


def _out(dev, n, out_c):
    import torch
    flat = torch.full((n * out_c * COLS + OUT_GUARD,), OUT_FILL, dtype=torch.float64, device=dev)
    return flat, flat[: n * out_c * COLS].view(n, out_c, COLS)


def _done(flat, n, out_c):
    host = flat.cpu().numpy()
    assert (host[n * out_c * COLS:] == OUT_FILL).all(), "the kernel wrote behind its output"
    return host[: n * out_c * COLS].reshape(n, out_c, COLS)


def plane_entry(ops, planes, bbox, cs, W, out_c, select=None, scratch=None, scratch2=None, skel_out=None, um=UM):
    """One launch of ``demia_mask_skeleton``: [n, out_c, 8]; position t takes the table rows and the words of mask ``select[t]``.
    ``cs`` None: the thin-only form (count, info and out NULL), which returns nothing and fills ``skel_out``."""
    import torch

    from deepemia_amd import _lib
    M, H, wpr = planes.shape
    n, sel_d, bb = M, None, bbox
    count = info = None
    if cs is not None:
        count, info = cs.count, cs.info
    if select is not None:
        sel_d = torch.tensor(list(select), dtype=torch.int32, device=planes.device)
        idx = sel_d.to(torch.int64)
        bb, n = bbox.index_select(0, idx), len(select)
        if cs is not None:
            count, info = cs.count.index_select(0, idx), cs.info.index_select(0, idx)
    scratch = torch.empty_like(planes) if scratch is None else scratch
    scratch2 = torch.empty_like(planes) if scratch2 is None else scratch2
    flat = out = None
    if cs is not None:
        flat, out = _out(planes.device, n, out_c)
    before = planes.clone()
    _lib.check(ops.lib.demia_mask_skeleton(_lib.ptr(sel_d), _lib.ptr(planes), _lib.ptr(scratch), _lib.ptr(bb), _lib.ptr(count), _lib.ptr(info),
                                           n, H, W, cs.C if cs is not None else 0, float(um), _lib.ptr(out), out_c if cs is not None else 0,
                                           _lib.ptr(scratch2), _lib.ptr(skel_out), ops._stream()), "demia_mask_skeleton")
    got = _done(flat, n, out_c) if cs is not None else None
    assert torch.equal(before, planes), "the kernel changed the mask words"
    return got


def _crop_scratch2(ops, rooms, hw, guard=64):
    """The second scratch of ``demia_crop_skeleton``: (words filled with the canary + a guard, offsets on the device, on the host, total)."""
    import torch
    rooms = np.ascontiguousarray(rooms, dtype=np.int32).reshape(-1, 4)
    off = np.zeros(len(rooms), dtype=np.int64)
    total = int(ops.lib.demia_crop_skeleton_scratch(rooms.ctypes.data, len(rooms), hw[0], hw[1], off.ctypes.data))
    return _canary(ops.device, total, guard), torch.from_numpy(off).to(ops.device), off, total


def crop_entry(ops, payload, room, offsets, bbox, cs, hw, out_c, scr, scr2, select=None, skel_out=None, um=UM):
    """One launch of ``demia_crop_skeleton`` over explicit tables (payload, room, offsets and both scratch offsets indexed by
    ``select[t]``); ``scr`` / ``scr2``: (words, offsets) of the two scratches.  ``cs`` None: the thin-only form."""
    import torch

    from deepemia_amd import _lib
    n, sel_d, bb = int(bbox.shape[0]), None, bbox
    count = info = None
    if cs is not None:
        count, info = cs.count, cs.info
    if select is not None:
        sel_d = torch.tensor(list(select), dtype=torch.int32, device=payload.device)
        idx = sel_d.to(torch.int64)
        bb, n = bbox.index_select(0, idx), len(select)
        if cs is not None:
            count, info = cs.count.index_select(0, idx), cs.info.index_select(0, idx)
    flat = out = None
    if cs is not None:
        flat, out = _out(payload.device, n, out_c)
    before = payload.clone()
    _lib.check(ops.lib.demia_crop_skeleton(_lib.ptr(sel_d), _lib.ptr(payload), _lib.ptr(room), _lib.ptr(offsets), _lib.ptr(bb), _lib.ptr(count),
                                           _lib.ptr(info), n, hw[0], hw[1], cs.C if cs is not None else 0, float(um), _lib.ptr(out),
                                           out_c if cs is not None else 0, _lib.ptr(scr[0]), _lib.ptr(scr[1]), _lib.ptr(scr2[0]),
                                           _lib.ptr(scr2[1]), _lib.ptr(skel_out), ops._stream()), "demia_crop_skeleton")
    got = _done(flat, n, out_c) if cs is not None else None
    assert torch.equal(before, payload), "the kernel changed the payload"
    return got


def _check_rows(name, got, cs_host, m, ref, um=UM):
    """Every contour row of mask m against the reference at the trace's own start pixel, as messages."""
    count, info = cs_host[0], cs_host[1]
    bad = []
    for c in range(int(count[m])):
        want = ref.values(int(info[m, c, 0]), int(info[m, c, 1]), um)
        bad += [(name, c, msg) for msg in SR.compare(got[m, c], want)]
    return bad


def _grown(tight, H, W):
    grown = tight.copy()
    ok = tight[:, 0] >= 0
    grown[ok] = np.stack([np.maximum(tight[ok, 0] - 7, 0), np.maximum(tight[ok, 1] - 40, 0), np.minimum(tight[ok, 2] + 3, H - 1),
                          np.minimum(tight[ok, 3] + 33, W - 1)], axis=1)
    return grown


# ------------------------------------------------------------------------------------------------- 1. the skeleton, bit for bit
def test_thinning_equals_the_reference_bit_for_bit_in_both_entries(ops, cases, refs):
    for name, c in cases.items():
        H, W = c.mask.shape
        wpr = (W + 31) // 32
        ops.set_frame_width(W)
        planes = ops.from_dense(c.mask[None])
        _, bbox = ops.area_bbox(planes)
        tight = bbox.cpu().numpy()
        ry0, ry1, wx0, wx1 = _region(tight[0], H, W)
        want = _pack(refs[name].skeleton)
        # planes: every word of the region holds the skeleton, no other word changes
        skel = _canary(ops.device, H * wpr, 64)
        plane_entry(ops, planes, bbox, None, W, 0, skel_out=skel)
        got = skel.cpu().numpy().view(np.uint32)
        assert (got[H * wpr:] == CANARY).all(), name
        got = got[: H * wpr].reshape(H, wpr)
        inside = np.zeros((H, wpr), bool)
        inside[ry0:ry1 + 1, wx0:wx1 + 1] = True
        assert np.array_equal(got[inside], want[inside]) and not want[~inside].any(), name
        assert (got[~inside] == CANARY).all(), name
        # ... and unpacked by the product it is the reference's skeleton
        assert np.array_equal(ops.to_dense(ops.skeleton(planes), W)[0], refs[name].skeleton), name
        # crops, in a tight and in a grown room: the words of the region that lie in the room, nothing else of the payload
        for what, rooms in (("tight", tight), ("grown", _grown(tight, H, W))):
            payload, room, offsets = _crop_tables(ops, c.mask[None], rooms)
            scr, scr2 = _crop_scratch(ops, rooms, (H, W)), _crop_scratch2(ops, rooms, (H, W))
            skel = _canary(ops.device, int(payload.numel()))
            crop_entry(ops, payload, room, offsets, bbox, None, (H, W), 0, scr, scr2, skel_out=skel)
            got = skel.cpu().numpy().view(np.uint32)
            y0, x0, y1, x1 = (int(v) for v in rooms[0])
            c0, c1 = x0 >> 5, x1 >> 5
            exp = np.full(got.shape, CANARY, dtype=np.uint32)
            view = exp[5: 5 + (y1 - y0 + 1) * (c1 - c0 + 1)].reshape(y1 - y0 + 1, c1 - c0 + 1)      # _crop_tables: a gap of 5 words in front
            ya, yb, ca, cb = max(ry0, y0), min(ry1, y1), max(wx0, c0), min(wx1, c1)
            view[ya - y0:yb - y0 + 1, ca - c0:cb - c0 + 1] = want[ya:yb + 1, ca:cb + 1]
            assert np.array_equal(got, exp), (name, what)
            for s in (scr, scr2):                                        # neither scratch is written behind its total
                assert (s[0].cpu().numpy().view(np.uint32)[s[3]:] == CANARY).all(), (name, what)
    # an empty mask writes nothing
    ops.set_frame_width(40)
    planes = ops.from_dense(np.zeros((1, 20, 40), bool))
    skel = _canary(ops.device, 40)
    plane_entry(ops, planes, ops.area_bbox(planes)[1], None, 40, 0, skel_out=skel)
    assert (skel.cpu().numpy().view(np.uint32) == CANARY).all()


def test_thinning_of_random_masks_in_one_launch(ops):
    """Noise and smoothed-noise blobs, 64 masks in one launch: their thinning ends at different pairs in different places, which is
    what the windows of the later pairs (the words the pair before changed, grown by two) have to get right."""
    rng = np.random.default_rng(31)
    H, W = 45, 75
    masks = np.zeros((64, H, W), bool)
    for k in range(64):
        if k % 2:
            f = SR.ndimage.gaussian_filter(rng.random((H, W)), sigma=float(rng.uniform(0.8, 3.0)))
            masks[k] = f > np.quantile(f, float(rng.uniform(0.2, 0.7)))
        else:
            masks[k] = rng.random((H, W)) < rng.uniform(0.3, 0.97)
    ops.set_frame_width(W)
    got = ops.to_dense(ops.skeleton(ops.from_dense(masks)), W)
    for k in range(64):
        assert np.array_equal(got[k], SR.thin(masks[k])[0]), k


# ------------------------------------------------------------------------------------------------------ 2. values vs reference
def test_values_vs_reference(ops, cases, refs):
    bad, rows = [], 0
    for name, c in cases.items():
        planes, bbox, cs = _trace(ops, c.mask[None])
        host = cs.host()
        n = int(host[0][0])
        assert n == len(refs[name].starts()) and (c.contours < 0 or n == c.contours), (name, n)
        got = plane_entry(ops, planes, bbox, cs, c.mask.shape[1], cs.C)
        bad += _check_rows(name, got, host, 0, refs[name])
        rows += n
        assert (got[0, n:] == 0).all(), name                            # slots without a contour hold zeros
        if c.known is not None:
            order = np.lexsort((host[1][0, :n, 0], host[1][0, :n, 1]))   # raster order of the starts
            for k, want in zip(order, c.known):
                assert tuple(int(v) for v in got[0, k, :5]) == want, (name, got[0, k])
    print(f"kernel against the reference: {rows} contours of {len(cases)} masks")
    assert not bad, bad
    # an empty mask and an empty box: zeros
    planes, bbox, cs = _trace(ops, np.zeros((1, 20, 40), bool))
    assert (plane_entry(ops, planes, bbox, cs, 40, 3) == 0).all()
    # a start pixel that is not set: zeros in that slot
    planes, bbox, cs = _trace(ops, cases["two_components"].mask[None])
    cs.info[0, 0, 0] = 99
    got = plane_entry(ops, planes, bbox, cs, cases["two_components"].mask.shape[1], 2)
    assert (got[0, 0] == 0).all() and got[0, 1, 0] > 0


# ---------------------------------------------------------------------------------------- 3. translation and layout invariance
OFFSETS = ((0, 0), (3, 1), (17, 31), (5, 32), (9, 33))


def _blob():
    """A blob with a 1-px zero margin of its own (so the frame never bounds it): an ellipse, a bar and a hole."""
    yy, xx = np.mgrid[0:50, 0:75]
    m = ((xx - 30) * 0.8 + (yy - 25) * 0.6) ** 2 / 27 ** 2 + (-(xx - 30) * 0.6 + (yy - 25) * 0.8) ** 2 / 14 ** 2 <= 1
    m[20:26, 30:73] = True
    m[22:25, 25:33] = False
    m[0, :] = m[-1, :] = False
    m[:, 0] = m[:, -1] = False
    return m


def test_translation_and_layout_invariance(ops):
    blob = _blob()
    H, W = 70, 118                                                      # a partial last word
    masks = np.zeros((len(OFFSETS), H, W), bool)
    for k, (oy, ox) in enumerate(OFFSETS):
        masks[k, oy:oy + blob.shape[0], ox:ox + blob.shape[1]] = blob
    planes, bbox, cs = _trace(ops, masks)
    host = cs.host()
    assert (host[0] == 1).all()
    got = plane_entry(ops, planes, bbox, cs, W, 2)
    bad = _check_rows("blob", got, host, 0, SR.Reference(masks[0]))
    assert not bad, bad
    assert got[0, 0, 0] > 20 and got[0, 0, 3] >= 2                      # a skeleton worth the name
    for k in range(len(OFFSETS)):
        assert (_bits(got[k, 0]) == _bits(got[0, 0])).all() and (got[k, 1] == 0).all(), k
    # a frame of whole words, the blob at the same offsets
    planes_w, bbox_w, cs_w = _trace(ops, np.concatenate([masks, np.zeros((len(OFFSETS), H, 128 - W), bool)], axis=2))
    got_w = plane_entry(ops, planes_w, bbox_w, cs_w, 128, 1)
    assert (_bits(got_w[:, 0]) == _bits(got[:, 0])).all()
    # other batch positions: under select with a repeat and a permutation, the words served from the first set
    sel = [4, 0, 2, 0, 3, 1]
    got_s = plane_entry(ops, planes, bbox, cs, W, 1, select=sel)
    assert (_bits(got_s[:, 0]) == _bits(got[sel, 0])).all()
    # the skeleton itself moves with the blob
    ops.set_frame_width(W)
    skel =ops.to_dense(ops.skeleton(planes, bbox), W)
    for k, (oy, ox) in enumerate(OFFSETS):
        assert np.array_equal(skel[k, oy:oy + blob.shape[0], ox:ox + blob.shape[1]], skel[0, :blob.shape[0], :blob.shape[1]]), k
        assert skel[k].sum() == got[0, 0, 0]
    # another um: integers unchanged
    alone = plane_entry(ops, planes, bbox, cs, W, 1, um=1.0)
    assert (alone[:, 0, :6] == got[:, 0, :6]).all() and alone[0, 0, 7] == got[0, 0, 5] / got[0, 0, 0]


def test_crop_words_equal_planes(ops, cases):
    import torch
    names = ["k_ring18_9", "six_components", "touches_all_edges", "two_components", "junction_Y", "nested_in_ring", "band_diagonal"]
    H, W = 150, 230
    at = [(3, 40), (50, 60), (109, 177), (0, 0), (80, 5), (20, 130), (75, 120)]          # touches_all_edges sits in the frame's corner
    masks = np.concatenate([_frame_of_cases(cases, names, H, W, at), np.zeros((1, H, W), bool)])      # + an empty mask
    planes, bbox, cs = _trace(ops, masks)
    want = plane_entry(ops, planes, bbox, cs, W, cs.max_count)
    assert int(cs.host()[0][1]) == 6 and int(cs.host()[0][-1]) == 0 and (want[-1] == 0).all()
    tight = bbox.cpu().numpy()
    assert tight[2].tolist() == [109, 177, 149, 229] and tight[-1, 0] == -1          # a room on the frame's edge, an empty room
    for what, rooms in (("tight", tight), ("grown", _grown(tight, H, W))):
        payload, room, offsets = _crop_tables(ops, masks, rooms)
        scr, scr2 = _crop_scratch(ops, rooms, (H, W)), _crop_scratch2(ops, rooms, (H, W))
        assert scr[3] == 0 and scr2[3] == 0                              # every region fits in LDS: the scratches are never touched
        got = crop_entry(ops, payload, room, offsets, bbox, cs, (H, W), cs.max_count, scr, scr2)
        assert (_bits(got) == _bits(want)).all(), what
        sel = [6, 1, 7, 3, 1]
        got_s = crop_entry(ops, payload, room, offsets, bbox, cs, (H, W), cs.max_count, scr, scr2, select=sel)
        assert (_bits(got_s) == _bits(want[sel])).all(), what
        for s in (scr, scr2):
            assert (s[0].cpu().numpy().view(np.uint32) == CANARY).all(), what
    # the product's own set of the same planes (rooms = tight boxes), through ContourSet
    from deepemia_amd.cropset import CropMaskSet
    cset = CropMaskSet.from_planes(ops, planes, W)
    ccs = cset.trace(max_contours=16, keep_words=True)
    assert torch.equal(ccs.count, cs.count)
    got = ccs.descriptor("skeleton", UM)
    for m in range(len(masks)):                                          # (a second trace may leave a mask's contours in other slots)
        n = int(cs.host()[0][m])
        a = got[m, :n][np.lexsort((ccs.host()[1][m, :n, 0], ccs.host()[1][m, :n, 1]))]
        b = want[m, :n][np.lexsort((cs.host()[1][m, :n, 0], cs.host()[1][m, :n, 1]))]
        assert (_bits(a) == _bits(b)).all(), m


# ------------------------------------------------------------------------------------------------------ 4. the scratch contract
def test_large_region_stays_inside_its_share_and_equals_the_lds_path(ops, cases, refs):
    import torch
    H, W = cases[SC.LARGE].mask.shape
    wpr = (W + 31) // 32
    # the same small mask twice: with its tight box (LDS) and with the whole frame as its box (a superset: the scratch path);
    # between them the large mask; and the small mask in a frame of its own
    small = cases["six_components"].mask
    placed = _frame_of_cases(cases, ["six_components"], H, W, [(200, 700)])[0]
    masks = np.stack([placed, cases[SC.LARGE].mask, placed])
    ops.set_frame_width(W)
    planes = ops.from_dense(masks)
    _, bbox = ops.area_bbox(planes)
    bbox[2] = torch.tensor([0, 0, H - 1, W - 1], dtype=torch.int32, device=bbox.device)
    assert (H + 2) * (wpr + 2) > LARGE_WORDS
    cs = ops.trace(planes, max_contours=16, bbox=bbox)
    host = cs.host()
    assert host[0].tolist() == [6, 1, 6]
    # planes: masks 1 and 2 work in their planes of both scratches; mask 0's planes and the guards stay untouched
    n = 3 * H * wpr
    s1, s2, skel = _canary(ops.device, n, 64), _canary(ops.device, n, 64), _canary(ops.device, n, 64)
    got = plane_entry(ops, planes, bbox, cs, W, 6, scratch=s1[:n].view(3, H, wpr), scratch2=s2[:n].view(3, H, wpr), skel_out=skel)
    for s in (s1, s2):
        after = s.cpu().numpy().view(np.uint32)
        assert (after[: H * wpr] == CANARY).all() and (after[n:] == CANARY).all()
        assert (after[H * wpr:2 * H * wpr] != CANARY).any() and (after[2 * H * wpr:n] != CANARY).any()
    assert not _check_rows(SC.LARGE, got, host, 1, refs[SC.LARGE])
    sk = skel.cpu().numpy().view(np.uint32)
    assert (sk[n:] == CANARY).all() and np.array_equal(sk[H * wpr:2 * H * wpr].reshape(H, wpr), _pack(refs[SC.LARGE].skeleton))
    assert np.array_equal(sk[2 * H * wpr:n].reshape(H, wpr), _pack(np.pad(refs["six_components"].skeleton,
                                                                          ((200, H - 200 - small.shape[0]), (700, W - 700 - small.shape[1])))))
    # the scratch path equals the LDS path: the same mask with its tight box, and in a small frame of its own
    p_small, b_small, cs_small = _trace(ops, small[None], C=16)
    lds = plane_entry(ops, p_small, b_small, cs_small, small.shape[1], 6)

    def by_start(rows, h, m):
        k = int(h[0][m])
        return rows[m, :k][np.lexsort((h[1][m, :k, 0], h[1][m, :k, 1]))]

    assert (_bits(by_start(got, host, 0)) == _bits(by_start(got, host, 2))).all()
    assert (_bits(by_start(got, host, 2)) == _bits(by_start(lds, cs_small.host(), 0))).all()
    # crops: rooms = the boxes given; masks 1 and 2 have a share of each scratch, two and one padded regions
    rooms = bbox.cpu().numpy()
    payload, room, offsets = _crop_tables(ops, masks, rooms)
    scr, scr2 = _crop_scratch(ops, rooms, (H, W)), _crop_scratch2(ops, rooms, (H, W))
    pn = (H + 2) * (wpr + 2)
    assert scr[3] == 4 * pn and scr2[3] == 2 * pn and scr2[2].tolist() == [0, 0, pn]
    got_c = crop_entry(ops, payload, room, offsets, bbox, cs, (H, W), 6, scr, scr2)
    assert (_bits(got_c) == _bits(got)).all()
    for s in (scr, scr2):
        after = s[0].cpu().numpy().view(np.uint32)
        assert (after[s[3]:] == CANARY).all() and (after[:s[3]] != CANARY).any()
    # the large mask served at position 0 of a one-mask launch, its words and its shares found through select
    one = crop_entry(ops, payload, room, offsets, bbox, cs, (H, W), 6, scr, scr2, select=[1])
    assert (_bits(one[0]) == _bits(got[1])).all()
    for s in (scr, scr2):
        assert (s[0].cpu().numpy().view(np.uint32)[s[3]:] == CANARY).all()


# ---------------------------------------------------------------------------------------------------- 5. slots vs on demand
def test_launch_slots_equals_on_demand(ops, cases, monkeypatch):
    import torch

    from deepemia_amd.cropset import CropMaskSet, CropPlanes, trace_chunks
    H, W = 150, 230
    six = _frame_of_cases(cases, ["six_components"], H, W, [(20, 33)])[0]
    few = _frame_of_cases(cases, ["two_components"], H, W, [(60, 90)])[0]
    ringm = _frame_of_cases(cases, ["nested_in_ring"], H, W, [(5, 160)])[0]
    ops.set_frame_width(W)
    for masks, fallback in ((np.stack([six, np.zeros_like(six), few]), True), (np.stack([few, np.zeros_like(few), ringm]), False)):
        planes = ops.from_dense(masks)
        cs = ops.trace(planes, max_contours=16, keep_words=True)
        cs.launch_measure(UM, slots=4)
        cs.launch("inscribed", UM, slots=4)
        cs.launch("skeleton", UM, slots=4)
        copies = _spy_copies(monkeypatch)
        cs.fetch(with_points=True)
        full = cs.descriptor("skeleton", UM)
        if not fallback:
            assert copies[0] == 1                                        # counts, tables, measurements, inscribed and skeleton values: ONE copy
        monkeypatch.undo()
        st = cs.launched["skeleton"]
        first = st.dev.cpu().numpy()
        assert (st.host is None) == fallback
        carried, st.host = st.host, None                                 # on demand, on the SAME tables, as if nothing had ridden along
        demand = cs.descriptor("skeleton", UM)
        picked = cs.descriptor("skeleton", UM, select=[2])
        st.host = carried
        n = int(cs.host()[0].max())
        assert (n > 4) == fallback and full.shape == demand.shape == (len(masks), n, COLS)
        assert (_bits(full) == _bits(demand)).all() and (_bits(first[:, :min(n, 4)]) == _bits(full[:, :4])).all()
        assert (_bits(picked[2]) == _bits(full[2])).all() and not picked[:2].any()
        recs = cs.records(um_pix=UM, descriptors=("skeleton",))
        assert all("skeleton" not in r for rs in cs.records(um_pix=UM) for r in rs)
        for mask, rs in zip(masks, recs):
            ref = SR.Reference(mask) if mask.any() else None
            for r in rs:
                assert not SR.compare(r["skeleton"], ref.values(r["start"][0], r["start"][1], UM)), r["start"]
    # mask_frame crop: chunks of two masks through a pool of two planes; the first two chunks hold a six-component mask and fall back
    # on demand only after every later chunk has reused the pool -- the words come from the set's payload (chunk 1: select = 2 + t)
    masks = np.stack([six, few, ringm, six[::-1, ::-1].copy(), ringm[:, ::-1].copy()])
    cset = CropMaskSet.from_planes(ops, ops.from_dense(masks), W)
    cp = CropPlanes(ops, (H, W), chunk=2)
    chunks = list(trace_chunks(cset, cp, max_contours=16, um_pix=UM, descriptors=("skeleton",)))
    assert [(f, n) for f, n, _ in chunks] == [(0, 2), (2, 2), (4, 1)]
    torch.cuda.synchronize()
    for f, n, cs in chunks:
        cs.fetch(with_points=True)
    assert [c[2].launched["skeleton"].host is None for c in chunks] == [True, True, False]
    for f, n, cs in chunks:
        recs = cs.records(um_pix=UM, descriptors=("skeleton",))
        for mask, rs in zip(masks[f:f + n], recs):
            ref = SR.Reference(mask)
            assert len(rs) == len(ref.starts())
            for r in rs:
                assert not SR.compare(r["skeleton"], ref.values(r["start"][0], r["start"][1], UM)), (f, r["start"])


# ------------------------------------------------------------------------------------- 6. the 12 + 10 + 8 other values untouched
def test_measure_shape_and_inscribed_values_are_untouched(ops, cases):
    from functools import partial

    import torch
    H, W = 150, 230
    masks = _frame_of_cases(cases, ["six_components", "ring", "dumbbell"], H, W, [(20, 33), (5, 160), (60, 10)])
    ops.set_frame_width(W)
    planes = ops.from_dense(masks)
    out = []
    for skel in (False, True):
        cs = ops.trace(planes, max_contours=16, keep_words=True)
        cs.launch_measure(UM, slots=8)
        cs.launch("shape", UM, slots=8)
        cs.launch("inscribed", UM, slots=8)
        if skel:
            cs.launch("skeleton", UM, slots=8)
        cs.fetch(with_points=True)
        assert ("skeleton" in cs.launched and cs.launched["skeleton"].host is not None) == skel
        order = [np.lexsort((cs.host()[1][m, :int(cs.host()[0][m]), 0], cs.host()[1][m, :int(cs.host()[0][m]), 1])) for m in range(len(masks))]
        out.append([tuple(torch.from_numpy(f(UM)[m][o].copy()) for f in (cs.measure, partial(cs.descriptor, "shape"), partial(cs.descriptor, "inscribed"))) for m, o in enumerate(order)])
    for a, b in zip(*out):
        assert [v.shape[1] for v in a] == [12, 10, 8] and all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------- 7. CLI
def _cli_runs(tmp_path, monkeypatch, runs):
    import main as cli
    from deepemia_amd.utils import config as C
    from test_gpu_cropset import DATASET, _set_frame, _write_tree

    ds_cfg = {"inference_overrides": {"confidence_mode": "manual",
                                      "class_specific_settings": {"class_0": {"confidence_threshold": 0.3, "iou_threshold": 0.6},
                                                                  "class_1": {"confidence_threshold": 0.35, "iou_threshold": 0.5}},
                                      "tile_settings": {"tile_size": 200, "overlap_ratio": 0.125, "upscale_factor": 1.0, "edge_filter_enabled": True},
                                      "spatial_constraints": {"enabled": True, "containment_rules": {1: 0}, "containment_threshold": 0.5}}}
    cfgdir, split = _write_tree(tmp_path, ds_cfg)
    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(cfgdir))
    monkeypatch.setenv("DEEPEMIA_OFFLINE", "1")
    monkeypatch.setenv("DEEPEMIA_WORKERS", "1")
    monkeypatch.chdir(tmp_path)
    names = ["measurements_results.csv", "R50_flip_results.csv"]
    outs = {}
    for frame, extra in runs:
        _set_frame(cfgdir, {"inference_overrides": dict(ds_cfg["inference_overrides"], **extra)}, frame)
        C.reset_cache()
        assert cli.main(["--task", "inference", "--dataset_name", DATASET, "--threshold", "0.3", "--no-gpu-check"]) == 0
        C.reset_cache()
        outs[frame, len(extra)] = {nm: (split / nm).read_bytes() for nm in names}
        for nm in names:
            (split / nm).unlink()
    return outs


def _rows(out):
    return list(csv.reader(io.StringIO(out["measurements_results.csv"].decode(), newline="")))


def test_cli_appends_five_columns_in_every_mask_frame(tmp_path, monkeypatch, gpu_device):
    from deepemia_amd.functions import inference as inf_mod
    on_cfg = {"skeleton_descriptors": True}
    outs = _cli_runs(tmp_path, monkeypatch, (("full", {}), ("full", on_cfg), ("crop", on_cfg), ("crop_direct", on_cfg)))
    off, on = outs["full", 0], outs["full", 1]
    off_rows, on_rows = _rows(off), _rows(on)
    assert len(off_rows) > 10 and all(len(r) == 20 for r in off_rows)
    assert on_rows[0] == inf_mod.CSV_HEADER + inf_mod.SKELETON_CSV_HEADER and all(len(r) == 25 for r in on_rows) and len(on_rows) == len(off_rows)
    # the first 20 fields of every line are the bytes of the run with the setting off; the other file is byte-identical
    off_lines, on_lines = off["measurements_results.csv"].decode().split("\r\n"), on["measurements_results.csv"].decode().split("\r\n")
    assert len(on_lines) == len(off_lines)
    for a, b in zip(on_lines, off_lines):
        assert a[:len(b)] == b and (a == b == "" or a[len(b)] == ","), (a, b)
    for frame in ("full", "crop", "crop_direct"):
        assert outs[frame, 1] == on, frame                               # both files, byte for byte: the five columns are equal in every frame
        assert outs[frame, 1]["R50_flip_results.csv"] == off["R50_flip_results.csv"]
    # plausible values: counts are integers, a skeleton has at least one pixel and is no longer than its links allow
    for r in on_rows[1:]:
        length, width, ends, branches, n = (float(x) for x in r[20:])
        assert n >= 1 and n == int(n) and ends == int(ends) and branches == int(branches) and width > 0
        assert length >= 0 and (n > 1) == (length > 0)                  # a connected skeleton of two pixels has a link


def test_cli_all_three_descriptor_settings_give_38_columns_in_every_frame(tmp_path, monkeypatch, gpu_device):
    from deepemia_amd.functions import inference as inf_mod
    all_on = {"skeleton_descriptors": True, "shape_descriptors": True, "inscribed_descriptors": True}
    outs = _cli_runs(tmp_path, monkeypatch, (("full", {"skeleton_descriptors": True}), ("full", all_on), ("crop", all_on), ("crop_direct", all_on)))
    five = _rows(outs["full", 1])
    for frame in ("full", "crop", "crop_direct"):
        rows = _rows(outs[frame, 3])
        assert rows[0] == inf_mod.CSV_HEADER + inf_mod.SHAPE_CSV_HEADER + inf_mod.INSCRIBED_CSV_HEADER + inf_mod.SKELETON_CSV_HEADER
        assert all(len(r) == 38 for r in rows) and [r[:20] + r[33:] for r in rows] == five, frame
        assert outs[frame, 3] == outs["full", 3], frame
