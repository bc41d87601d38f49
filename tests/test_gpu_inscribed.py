"""``demia_mask_inscribed`` / ``demia_crop_inscribed`` -- the largest inscribed circle and the distance-based thickness per contour
-- against the reference of ``tests/inscribed_ref.py`` on the masks of ``tests/inscribed_cases.py``, traced by the product's own
tracer; then position and layout invariance, the crop entry against the plane entry, the scratch contract, ``ContourSet`` and the
CLI.  Values 0-4 (R2, cx, cy, N, SD2) are asked exactly; 5-7 within relative ``8 * 2^-53`` (``inscribed_ref.REL_TOL``)."""
import csv
import io

import numpy as np
import pytest

import inscribed_cases as IC
import inscribed_ref as IR

pytestmark = pytest.mark.gpu

UM = 0.37
COLS = IR.INSCRIBED_COLS
OUT_FILL = -7.25
OUT_GUARD = 6 * COLS
CANARY = 0x5A5A5A5A
LARGE_WORDS = 8192                                                       # the tracer's large LDS buffer (words per region buffer)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def ops(gpu_device):
    from deepemia_amd.maskset import MaskOps
    return MaskOps(gpu_device)


@pytest.fixture(scope="module")
def cases():
    return IC.by_name()


@pytest.fixture(scope="module")
def refs(cases):
    """name -> Reference (D2 and components), computed once and shared."""
    return {name: IR.Reference(c.mask) for name, c in cases.items()}


def _trace(ops, masks, C=64):
    """Planes, tight boxes and the trace of a stack of dense masks [M, H, W]."""
    masks = np.asarray(masks, dtype=bool)
    ops.set_frame_width(masks.shape[2])
    planes = ops.from_dense(masks)
    _, bbox = ops.area_bbox(planes)
    cs = ops.trace(planes, max_contours=C, bbox=bbox)
    cs.host()
    return planes, bbox, cs


def _out(dev, n, out_c):
    import torch
    flat = torch.full((n * out_c * COLS + OUT_GUARD,), OUT_FILL, dtype=torch.float64, device=dev)
    return flat, flat[: n * out_c * COLS].view(n, out_c, COLS)


def _done(flat, n, out_c):
    host = flat.cpu().numpy()
    assert (host[n * out_c * COLS:] == OUT_FILL).all(), "the kernel wrote behind its output"
    return host[: n * out_c * COLS].reshape(n, out_c, COLS)


def plane_entry(ops, planes, bbox, cs, W, out_c, select=None, scratch=None, um=UM):
    """One launch of ``demia_mask_inscribed``: [n, out_c, 8]; position t takes the table rows and the words of mask ``select[t]``."""
    import torch

    from deepemia_amd import _lib
    M, H, wpr = planes.shape
    count, info, bb, sel_d, n = cs.count, cs.info, bbox, None, M
    if select is not None:
        sel_d = torch.tensor(list(select), dtype=torch.int32, device=planes.device)
        idx = sel_d.to(torch.int64)
        count, info, bb, n = cs.count.index_select(0, idx), cs.info.index_select(0, idx), bbox.index_select(0, idx), len(select)
    if scratch is None:
        scratch = torch.empty_like(planes)
    flat, out = _out(planes.device, n, out_c)
    before = planes.clone()
    _lib.check(ops.lib.demia_mask_inscribed(_lib.ptr(sel_d), _lib.ptr(planes), _lib.ptr(scratch), _lib.ptr(bb), _lib.ptr(count), _lib.ptr(info),
                                            n, H, W, cs.C, float(um), _lib.ptr(out), out_c, ops._stream()), "demia_mask_inscribed")
    got = _done(flat, n, out_c)
    assert torch.equal(before, planes), "the kernel changed the mask words"
    return got


def crop_entry(ops, payload, room, offsets, bbox, cs, hw, out_c, scratch, scratch_off, select=None, um=UM):
    """One launch of ``demia_crop_inscribed`` over explicit tables (payload, room, offsets and scratch_off indexed by ``select[t]``)."""
    import torch

    from deepemia_amd import _lib
    count, info, bb, sel_d, n = cs.count, cs.info, bbox, None, int(cs.count.shape[0])
    if select is not None:
        sel_d = torch.tensor(list(select), dtype=torch.int32, device=payload.device)
        idx = sel_d.to(torch.int64)
        count, info, bb, n = cs.count.index_select(0, idx), cs.info.index_select(0, idx), bbox.index_select(0, idx), len(select)
    flat, out = _out(payload.device, n, out_c)
    before = payload.clone()
    _lib.check(ops.lib.demia_crop_inscribed(_lib.ptr(sel_d), _lib.ptr(payload), _lib.ptr(room), _lib.ptr(offsets), _lib.ptr(bb), _lib.ptr(count),
                                            _lib.ptr(info), n, hw[0], hw[1], cs.C, float(um), _lib.ptr(out), out_c, _lib.ptr(scratch),
                                            _lib.ptr(scratch_off), ops._stream()), "demia_crop_inscribed")
    got = _done(flat, n, out_c)
    assert torch.equal(before, payload), "the kernel changed the payload"
    return got


def _check_rows(name, got, cs_host, m, ref, um=UM):
    """Every contour row of mask m against the reference at the trace's own start pixel; returns (messages, worst relative difference)."""
    count, info = cs_host[0], cs_host[1]
    bad, worst = [], 0.0
    for c in range(int(count[m])):
        sx, sy = int(info[m, c, 0]), int(info[m, c, 1])
        want = ref.values(sx, sy, um)
        bad += [(name, c, msg) for msg in IR.compare(got[m, c], want)]
        worst = max(worst, IR.worst_rel(got[m, c], want))
    return bad, worst


# ------------------------------------------------------------------------------------------------------ 1. values vs reference
def test_values_vs_reference(ops, cases, refs):
    bad, worst, rows = [], 0.0, 0
    for name, c in cases.items():
        planes, bbox, cs = _trace(ops, c.mask[None])
        host = cs.host()
        n = int(host[0][0])
        assert n == len(refs[name].starts()) and (c.contours < 0 or n == c.contours), (name, n)
        got = plane_entry(ops, planes, bbox, cs, c.mask.shape[1], cs.C)
        b, w = _check_rows(name, got, host, 0, refs[name])
        bad += b
        worst = max(worst, w)
        rows += n
        assert (got[0, n:] == 0).all(), name                            # slots without a contour hold zeros
        if c.known is not None:
            order = np.lexsort((host[1][0, :n, 0], host[1][0, :n, 1]))   # raster order of the starts
            for k, want in zip(order, c.known):
                assert tuple(int(v) for v in got[0, k, :5]) == want, (name, got[0, k])
    print(f"kernel against the reference, {rows} contours of {len(cases)} masks: worst relative difference of values 5..7 "
          f"{worst:.3g} (bound {IR.REL_TOL:.3g})")
    assert not bad, bad
    # an empty mask and an empty box: zeros
    planes, bbox, cs = _trace(ops, np.zeros((1, 20, 40), bool))
    assert (plane_entry(ops, planes, bbox, cs, 40, 3) == 0).all()


# ---------------------------------------------------------------------------------------- 2. translation and layout invariance
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
    ref = IR.Reference(masks[0])
    bad, _ = _check_rows("blob", got, host, 0, ref)
    assert not bad, bad

    def same_up_to_offset(row, k, what):
        oy, ox = OFFSETS[k]
        assert (row[[0, 3, 4]] == got[0, 0, [0, 3, 4]]).all(), (what, k)
        assert row[1] == got[0, 0, 1] + ox and row[2] == got[0, 0, 2] + oy, (what, k, row, got[0, 0])
        assert (_bits(row[5:]) == _bits(got[0, 0, 5:])).all(), (what, k)

    for k in range(len(OFFSETS)):
        same_up_to_offset(got[k, 0], k, "batch")
        assert (got[k, 1] == 0).all()
    # other batch positions: the masks reversed and re-traced; under select, the words served from the first set
    planes_r, bbox_r, cs_r = _trace(ops, masks[::-1].copy())
    got_r = plane_entry(ops, planes_r, bbox_r, cs_r, W, 1)
    sel = [4, 0, 2]
    got_s = plane_entry(ops, planes, bbox, cs, W, 1, select=sel)
    for k in range(len(OFFSETS)):
        same_up_to_offset(got_r[len(OFFSETS) - 1 - k, 0], k, "reversed")
    for t, k in enumerate(sel):
        same_up_to_offset(got_s[t, 0], k, "select")
    # each mask alone, and at another um: integers unchanged
    alone = plane_entry(ops, planes[3:4].contiguous(), bbox[3:4].contiguous(), _trace(ops, masks[3:4])[2], W, 1, um=1.0)
    assert (alone[0, 0, :5] == got[3, 0, :5]).all() and abs(alone[0, 0, 5] - 2.0 * np.sqrt(got[3, 0, 0])) <= IR.REL_TOL * alone[0, 0, 5]


# ------------------------------------------------------------------------------------------------- 3. crop words equal planes
def _frame_of_cases(cases, names, H, W, at):
    masks = np.zeros((len(names), H, W), bool)
    for k, (nm, (oy, ox)) in enumerate(zip(names, at)):
        m = cases[nm].mask
        masks[k, oy:oy + m.shape[0], ox:ox + m.shape[1]] = m
    return masks


def _crop_tables(ops, masks, rooms, gap=5):
    """payload (all ones where no mask's own word lies: gaps in front of, between and behind the rooms), room, offsets on the
    device for the dense masks cropped to ``rooms``; words laid out exactly as the crop-framed sets lay them out."""
    import torch
    rooms = np.asarray(rooms, dtype=np.int32).reshape(-1, 4)
    words, offs, pos = [], [], gap
    for m, (y0, x0, y1, x1) in zip(masks, rooms.tolist()):
        offs.append(pos)
        if y0 < 0:
            continue
        c0, c1 = x0 >> 5, x1 >> 5
        sub = np.zeros((y1 - y0 + 1, (c1 - c0 + 1) * 32), bool)
        x_hi = min((c1 + 1) * 32, m.shape[1])
        sub[:, : x_hi - c0 * 32] = m[y0:y1 + 1, c0 * 32:x_hi]
        w = np.packbits(sub.reshape(sub.shape[0], -1, 32), axis=-1, bitorder="little").view(np.uint32).reshape(-1)
        words.append((pos, w))
        pos += len(w) + gap
    payload = np.full(pos, 0xFFFFFFFF, dtype=np.uint32)
    for p, w in words:
        payload[p:p + len(w)] = w
    dev = ops.device
    return (torch.from_numpy(payload.view(np.int32)).to(dev), torch.from_numpy(rooms).to(dev),
            torch.from_numpy(np.asarray(offs, dtype=np.int64)).to(dev))


def _crop_scratch(ops, rooms, hw, guard=64):
    """(scratch filled with the canary + a guard behind it, scratch_off on the device, offsets on the host, total words)."""
    import torch
    rooms = np.ascontiguousarray(rooms, dtype=np.int32).reshape(-1, 4)
    off = np.zeros(len(rooms), dtype=np.int64)
    total = int(ops.lib.demia_crop_contour_scratch(rooms.ctypes.data, len(rooms), hw[0], hw[1], off.ctypes.data))
    scratch = torch.from_numpy(np.full(total + guard, CANARY, dtype=np.uint32).view(np.int32)).to(ops.device)
    return scratch, torch.from_numpy(off).to(ops.device), off, total


def test_crop_words_equal_planes(ops, cases):
    import torch
    names = ["ring", "six_components", "touches_all_edges", "two_components", "disc", "nested_in_ring", "c_shape"]
    H, W = 150, 230
    at = [(3, 40), (50, 60), (109, 177), (0, 0), (80, 5), (20, 130), (75, 150)]          # touches_all_edges sits in the frame's corner
    masks = np.concatenate([_frame_of_cases(cases, names, H, W, at), np.zeros((1, H, W), bool)])      # + an empty mask
    planes, bbox, cs = _trace(ops, masks)
    want = plane_entry(ops, planes, bbox, cs, W, cs.max_count)
    assert int(cs.host()[0][1]) == 6 and int(cs.host()[0][-1]) == 0 and (want[-1] == 0).all()
    tight = bbox.cpu().numpy()
    assert tight[2].tolist() == [109, 177, 149, 229] and tight[-1, 0] == -1          # a room on the frame's edge, an empty room
    grown = tight.copy()
    ok = tight[:, 0] >= 0
    grown[ok] = np.stack([np.maximum(tight[ok, 0] - 7, 0), np.maximum(tight[ok, 1] - 40, 0), np.minimum(tight[ok, 2] + 3, H - 1),
                          np.minimum(tight[ok, 3] + 33, W - 1)], axis=1)
    for what, rooms in (("tight", tight), ("grown", grown)):
        payload, room, offsets = _crop_tables(ops, masks, rooms)
        scratch, soff, _, total = _crop_scratch(ops, rooms, (H, W))
        assert total == 0                                                # every region fits in LDS: the scratch is never touched
        got = crop_entry(ops, payload, room, offsets, bbox, cs, (H, W), cs.max_count, scratch, soff)
        assert (_bits(got) == _bits(want)).all(), what
        assert (scratch.cpu().numpy().view(np.uint32) == CANARY).all(), what
        sel = [6, 1, 7, 3]
        got_s = crop_entry(ops, payload, room, offsets, bbox, cs, (H, W), cs.max_count, scratch, soff, select=sel)
        assert (_bits(got_s) == _bits(want[sel])).all(), what
    # the product's own set of the same planes (rooms = tight boxes), through ContourSet
    from deepemia_amd.cropset import CropMaskSet
    cset = CropMaskSet.from_planes(ops, planes, W)
    ccs = cset.trace(max_contours=16, keep_words=True)
    assert torch.equal(ccs.count, cs.count)
    got = ccs.descriptor("inscribed", UM)
    for m in range(len(masks)):                                          # (a second trace may leave a mask's contours in other slots)
        n = int(cs.host()[0][m])
        a = got[m, :n][np.lexsort((ccs.host()[1][m, :n, 0], ccs.host()[1][m, :n, 1]))]
        b = want[m, :n][np.lexsort((cs.host()[1][m, :n, 0], cs.host()[1][m, :n, 1]))]
        assert (_bits(a) == _bits(b)).all(), m


# ------------------------------------------------------------------------------------------------------ 4. the scratch contract
def test_large_region_uses_scratch_only_inside_its_share(ops, cases, refs):
    import torch
    big, small = cases[IC.LARGE].mask, np.zeros_like(cases[IC.LARGE].mask)
    small[200:230, 700:790] = True
    small[5:9, 5:9] = True
    H, W = big.shape
    masks = np.stack([small, big, small[::-1].copy()])
    planes, bbox, cs = _trace(ops, masks)
    host = cs.host()
    assert host[0].tolist() == [2, 1, 2] and (H + 2) * ((W + 31) // 32 + 2) > LARGE_WORDS
    wpr = planes.shape[2]
    # planes: the scratch plane of the big mask is its share; the small masks' planes and the guard stay untouched
    flat = torch.from_numpy(np.full(3 * H * wpr + 64, CANARY, dtype=np.uint32).view(np.int32)).to(ops.device)
    got = plane_entry(ops, planes, bbox, cs, W, 2, scratch=flat[: 3 * H * wpr].view(3, H, wpr))
    after = flat.cpu().numpy().view(np.uint32)
    assert (after[: H * wpr] == CANARY).all() and (after[2 * H * wpr:] == CANARY).all() and (after[H * wpr:2 * H * wpr] != CANARY).any()
    assert tuple(int(v) for v in got[1, 0, :5]) == cases[IC.LARGE].known[0]
    for m, mask in enumerate(masks):
        bad, _ = _check_rows(m, got, host, m, refs[IC.LARGE] if m == 1 else IR.Reference(mask))
        assert not bad, bad
    # crops: rooms = tight boxes; only the big mask has a share, [off, off + 2 * padded region)
    rooms = bbox.cpu().numpy()
    payload, room, offsets = _crop_tables(ops, masks, rooms)
    scratch, soff, off_h, total = _crop_scratch(ops, rooms, (H, W))
    pn = (H + 2) * (wpr + 2)
    assert total == 2 * pn and off_h.tolist() == [0, 0, total]
    got_c = crop_entry(ops, payload, room, offsets, bbox, cs, (H, W), 2, scratch, soff)
    assert (_bits(got_c) == _bits(got)).all()
    after = scratch.cpu().numpy().view(np.uint32)
    assert (after[total:] == CANARY).all() and (after[:total] != CANARY).any()
    # the big mask served at position 0 of a one-mask launch, its words and its share found through select
    one = crop_entry(ops, payload, room, offsets, bbox, cs, (H, W), 2, scratch, soff, select=[1])
    assert (_bits(one[0]) == _bits(got[1])).all()
    assert (scratch.cpu().numpy().view(np.uint32)[total:] == CANARY).all()


# ---------------------------------------------------------------------------------------------------- 5. slots vs on demand
def _spy_copies(monkeypatch):
    import torch
    n = [0]
    cpu = torch.Tensor.cpu

    def spy(self, *a, **k):
        n[0] += 1
        return cpu(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "cpu", spy)
    return n


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
        copies = _spy_copies(monkeypatch)
        cs.fetch(with_points=True)
        full = cs.descriptor("inscribed", UM)
        if not fallback:
            assert copies[0] == 1                                        # counts, tables, measurements and inscribed values: ONE copy
        monkeypatch.undo()
        st = cs.launched["inscribed"]
        first = st.dev.cpu().numpy()
        assert (st.host is None) == fallback
        carried, st.host = st.host, None                                 # on demand, on the SAME tables, as if nothing had ridden along
        demand = cs.descriptor("inscribed", UM)
        picked = cs.descriptor("inscribed", UM, select=[2])
        st.host = carried
        n = int(cs.host()[0].max())
        assert (n > 4) == fallback and full.shape == demand.shape == (len(masks), n, COLS)
        assert (_bits(full) == _bits(demand)).all() and (_bits(first[:, :min(n, 4)]) == _bits(full[:, :4])).all()
        assert (_bits(picked[2]) == _bits(full[2])).all() and not picked[:2].any()
        recs = cs.records(um_pix=UM, descriptors=("inscribed",))
        assert all("inscribed" not in r for rs in cs.records(um_pix=UM) for r in rs)
        for mask, rs in zip(masks, recs):
            ref = IR.Reference(mask) if mask.any() else None
            for r in rs:
                assert not IR.compare(r["inscribed"], ref.values(r["start"][0], r["start"][1], UM)), r["start"]
    # mask_frame crop: chunks of two masks through a pool of two planes; the first two chunks hold a six-component mask and fall back
    # on demand only after every later chunk has reused the pool -- the words come from the set's payload (chunk 1: select = 2 + t)
    masks = np.stack([six, few, ringm, six[::-1, ::-1].copy(), ringm[:, ::-1].copy()])
    cset = CropMaskSet.from_planes(ops, ops.from_dense(masks), W)
    cp = CropPlanes(ops, (H, W), chunk=2)
    chunks = list(trace_chunks(cset, cp, max_contours=16, um_pix=UM, descriptors=("inscribed",)))
    assert [(f, n) for f, n, _ in chunks] == [(0, 2), (2, 2), (4, 1)]
    torch.cuda.synchronize()
    for f, n, cs in chunks:
        cs.fetch(with_points=True)
    assert [c[2].launched["inscribed"].host is None for c in chunks] == [True, True, False]
    for f, n, cs in chunks:
        recs = cs.records(um_pix=UM, descriptors=("inscribed",))
        for mask, rs in zip(masks[f:f + n], recs):
            ref = IR.Reference(mask)
            assert len(rs) == len(ref.starts())
            for r in rs:
                assert not IR.compare(r["inscribed"], ref.values(r["start"][0], r["start"][1], UM)), (f, r["start"])


# ----------------------------------------------------------------------------------------- 6. the 12 + 10 values untouched
def test_measure_and_shape_values_are_untouched(ops, cases):
    import torch
    H, W = 150, 230
    masks = _frame_of_cases(cases, ["six_components", "ring", "dumbbell"], H, W, [(20, 33), (5, 160), (60, 10)])
    ops.set_frame_width(W)
    planes = ops.from_dense(masks)
    out = []
    for insc in (False, True):
        cs = ops.trace(planes, max_contours=16, keep_words=insc)
        cs.launch_measure(UM, slots=8)
        cs.launch("shape", UM, slots=8)
        if insc:
            cs.launch("inscribed", UM, slots=8)
        cs.fetch(with_points=True)
        order = [np.lexsort((cs.host()[1][m, :int(cs.host()[0][m]), 0], cs.host()[1][m, :int(cs.host()[0][m]), 1])) for m in range(len(masks))]
        out.append([(torch.from_numpy(cs.measure(UM)[m][o].copy()), torch.from_numpy(cs.descriptor("shape", UM)[m][o].copy())) for m, o in enumerate(order)])
    for (v0, s0), (v1, s1) in zip(*out):
        assert v0.shape[1] == 12 and s0.shape[1] == 10 and torch.equal(v0, v1) and torch.equal(s0, s1)


# ------------------------------------------------------------------------------------------------------------------- 7. CLI
def test_cli_appends_six_columns_in_every_mask_frame(tmp_path, monkeypatch, gpu_device):
    import main as cli
    from deepemia_amd.functions import inference as inf_mod
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
    for frame, extra in (("full", {}), ("full", {"inscribed_descriptors": True}), ("crop", {"inscribed_descriptors": True}),
                         ("crop_direct", {"inscribed_descriptors": True}),
                         ("crop", {"inscribed_descriptors": True, "shape_descriptors": True})):
        _set_frame(cfgdir, {"inference_overrides": dict(ds_cfg["inference_overrides"], **extra)}, frame)
        C.reset_cache()
        assert cli.main(["--task", "inference", "--dataset_name", DATASET, "--threshold", "0.3", "--no-gpu-check"]) == 0
        C.reset_cache()
        outs[frame, len(extra)] = {nm: (split / nm).read_bytes() for nm in names}
        for nm in names:
            (split / nm).unlink()

    def rows_of(key):
        return list(csv.reader(io.StringIO(outs[key]["measurements_results.csv"].decode(), newline="")))

    off, on = outs["full", 0], outs["full", 1]
    off_rows, on_rows = rows_of(("full", 0)), rows_of(("full", 1))
    assert len(off_rows) > 10 and all(len(r) == 20 for r in off_rows)
    assert on_rows[0] == inf_mod.CSV_HEADER + inf_mod.INSCRIBED_CSV_HEADER and all(len(r) == 26 for r in on_rows) and len(on_rows) == len(off_rows)
    # the first 20 fields of every line are the bytes of the run with the setting off; the other file is byte-identical
    off_lines, on_lines = off["measurements_results.csv"].decode().split("\r\n"), on["measurements_results.csv"].decode().split("\r\n")
    assert len(on_lines) == len(off_lines)
    for a, b in zip(on_lines, off_lines):
        assert a[:len(b)] == b and (a == b == "" or a[len(b)] == ","), (a, b)
    for frame in ("full", "crop", "crop_direct"):
        assert outs[frame, 1] == on, frame                               # both files, byte for byte: the six columns are equal in every frame
        assert outs[frame, 1]["R50_flip_results.csv"] == off["R50_flip_results.csv"]
    # plausible values: integers where the definition says so, the diameter from R2 ...
    for r in on_rows[1:]:
        d, cx, cy, rms, ratio, n = (float(x) for x in r[20:])
        assert d > 0 and cx == int(cx) and cy == int(cy) and n == int(n) and n >= 1 and 0 < rms <= d / 2 + 1e-9 and 0 < ratio < 1.2
    # both settings: 33 columns, shape first
    both = rows_of(("crop", 2))
    assert both[0] == inf_mod.CSV_HEADER + inf_mod.SHAPE_CSV_HEADER + inf_mod.INSCRIBED_CSV_HEADER and all(len(r) == 33 for r in both)
    assert [r[:20] + r[27:] for r in both] == on_rows
    assert outs["crop", 2]["R50_flip_results.csv"] == off["R50_flip_results.csv"]
