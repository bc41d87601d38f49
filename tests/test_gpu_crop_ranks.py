"""Crop-framed masks across ranks (``inference_settings.rank_exchange: crops``): ``demia_crop_reroom`` against a restatement on dense
arrays, ``CropMaskSet.to_table`` / ``from_table`` against the instance tables of the same masks' planes, the memory of the exchange,
and ``gather_and_merge`` / the tile pipeline / the CLI in both forms.  Every comparison is exact: both forms hold the same bits.

Boxes are (y0, x0, y1, x1) everywhere, as in the C ABI."""
import json
import os
import socket
import types

import numpy as np
import pytest
import torch
import yaml

from test_gpu_cropset import DATASET, _blob_planes, _loose_set, _write_tree

pytestmark = pytest.mark.gpu

H, W = 320, 417           # W is no multiple of 32: 14 words per row, the last one partly used; a full mask is 4480 words: two slabs
WPR = (W + 31) // 32
GUARD = -1                # 0xFFFFFFFF: what the destination holds before the launch, and the word behind it after


@pytest.fixture(scope="module")
def ops(gpu_device):
    from deepemia_amd.maskset import MaskOps
    return MaskOps(gpu_device)


@pytest.fixture(scope="module")
def env(ops):
    """~40 blobs + the hand-made cases, as planes and as a set with grown rooms."""
    hand = np.zeros((6, H, W), bool)
    hand[0, 100, 77] = True                         # a single pixel
    hand[1, 10:20, 64:96] = True                    # x0 % 32 == 0 and x1 % 32 == 31
    hand[2, 50:60, 30:71] = True                    # crosses two word boundaries
    hand[3, 300:H, 400:W] = True                    # on the right and bottom frame edges
    hand[5] = True                                  # fills the frame (hand[4] stays empty)
    ops.set_frame_width(W)
    planes = torch.cat([_blob_planes(ops, 40, H, W, 61), ops.from_dense(hand).contiguous()]).contiguous()
    cs, area, bbox = _loose_set(ops, planes, W, 62)
    return dict(planes=planes, P=planes.cpu().numpy().view(np.uint32), cs=cs, area=area, bbox=bbox, bbox_h=bbox.cpu().numpy(),
                area_h=area.cpu().numpy(), n=int(planes.shape[0]))


def _restated(P, src_room, dst_room, index):
    """The contract on dense word grids: mask index[i] as its source room holds it (zero outside that room), read through the
    window of dst_room[i]."""
    out = [np.zeros(0, np.uint32)]
    for i, j in enumerate(index):
        if dst_room[i, 0] < 0:
            continue
        G = np.zeros_like(P[j])
        if src_room[j, 0] >= 0:
            y0, x0, y1, x1 = src_room[j]
            G[y0:y1 + 1, x0 >> 5:(x1 >> 5) + 1] = P[j][y0:y1 + 1, x0 >> 5:(x1 >> 5) + 1]
        y0, x0, y1, x1 = dst_room[i]
        out.append(G[y0:y1 + 1, x0 >> 5:(x1 >> 5) + 1].ravel())
    return np.concatenate(out)


def _reroom_into_filled(ops, src, dst_room, index=None):
    """``demia_crop_reroom`` called directly, into a destination pre-filled with 0xFFFFFFFF with one guard word behind it."""
    from deepemia_amd import _lib
    from deepemia_amd.cropset import CropMaskSet, room_lengths
    sel = torch.arange(len(dst_room), device=ops.device) if index is None else torch.from_numpy(np.asarray(index, np.int64)).to(ops.device)
    out = CropMaskSet(ops, src.hw, dst_room, None, src.bbox.index_select(0, sel), src.area.index_select(0, sel))
    out.payload = torch.full((out.words + 1,), GUARD, dtype=torch.int32, device=ops.device)
    _lib.check(ops.lib.demia_crop_reroom(_lib.ptr(src.payload), _lib.ptr(src.room), _lib.ptr(src.offsets), _lib.ptr(None if index is None else sel),
                                         _lib.ptr(out.room), _lib.ptr(out.offsets), len(dst_room), int(room_lengths(dst_room).max()),
                                         _lib.ptr(out.payload), ops._stream()), "demia_crop_reroom")
    return out


def _contains(room, box):
    return (box[:, 0] < 0) | ((room[:, 0] >= 0) & (room[:, 0] <= box[:, 0]) & (room[:, 1] <= box[:, 1]) & (room[:, 2] >= box[:, 2]) & (room[:, 3] >= box[:, 3]))


def _rooms(env, kind):
    src_room, bb = env["cs"].room_h, env["bbox_h"]
    ok = src_room[:, 0] >= 0
    if kind == "tight":
        return bb.copy()
    room = src_room.copy()
    if kind == "grown":                             # beyond the source rooms on every side (where the frame leaves space)
        room[ok, 0] = np.maximum(room[ok, 0] - 5, 0); room[ok, 1] = np.maximum(room[ok, 1] - 40, 0)
        room[ok, 2] = np.minimum(room[ok, 2] + 7, H - 1); room[ok, 3] = np.minimum(room[ok, 3] + 33, W - 1)
        return room
    # partly: the tight box moved down and to the right by half its size + 3 rows / 35 columns, clipped -- it overlaps the source
    # room without containing the box; every fifth mask keeps a containing room, and one non-empty mask gets an empty room
    dy, dx = (bb[:, 2] - bb[:, 0]) // 2 + 3, (bb[:, 3] - bb[:, 1]) // 2 + 35
    room = np.stack([np.minimum(bb[:, 0] + dy, H - 1), np.minimum(bb[:, 1] + dx, W - 1), np.minimum(bb[:, 2] + dy, H - 1),
                     np.minimum(bb[:, 3] + dx, W - 1)], axis=1).astype(np.int32)
    room[::5] = src_room[::5]
    room[~ok] = -1
    room[7] = -1
    return room


# --------------------------------------------------------------------------------------------------------------- reroom
@pytest.mark.parametrize("kind", ["tight", "grown", "partly"])
def test_reroom_equals_the_restatement_on_dense_arrays(ops, env, kind):
    from deepemia_amd.cropset import room_lengths
    cs, P, n = env["cs"], env["P"], env["n"]
    dst_room = _rooms(env, kind)
    assert int(room_lengths(dst_room).max()) > 4096 and int(room_lengths(cs.room_h).max()) > 4096          # more than one slab
    out = _reroom_into_filled(ops, cs, dst_room)
    got = out.payload.cpu().numpy().view(np.uint32)
    want = _restated(P, cs.room_h, dst_room, np.arange(n))
    assert out.words == len(want) > 0 and np.array_equal(got[:-1], want)
    assert got[-1] == 0xFFFFFFFF                                                  # the word behind the payload
    inside = _contains(dst_room, env["bbox_h"])
    if kind == "partly":
        assert 5 < int(inside.sum()) < n - 5 and env["area_h"][7] > 0 and int((want != 0).sum()) > 0
    else:
        assert inside.all()
    it = torch.from_numpy(np.nonzero(inside)[0]).to(ops.device)
    assert torch.equal(out.to_planes()[it], env["planes"][it])
    # ... and the methods: one launch into a fresh payload
    via = cs.reroom(dst_room)
    assert np.array_equal(via.payload[:via.words].cpu().numpy().view(np.uint32), want) and np.array_equal(via.room_h, dst_room)
    assert torch.equal(via.bbox, cs.bbox) and torch.equal(via.area, cs.area)


def test_reroom_through_an_index_with_a_repeat(ops, env):
    cs, n = env["cs"], env["n"]
    index = np.random.default_rng(63).permutation(n).astype(np.int64)
    index[3] = index[0]
    index = np.concatenate([index, [n - 1, 2]])                                  # the frame-filling mask once more, an empty one
    dst_room = env["bbox_h"][index]
    out = _reroom_into_filled(ops, cs, dst_room, index)
    got = out.payload.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:-1], _restated(env["P"], cs.room_h, dst_room, index)) and got[-1] == 0xFFFFFFFF
    assert torch.equal(out.to_planes(), env["planes"][torch.from_numpy(index).to(ops.device)])


def test_tighten_is_reroom_to_the_boxes_and_itself_when_they_are_the_rooms(ops, env):
    cs = env["cs"]
    tight = cs.tighten(env["bbox_h"])
    assert tight is not cs and np.array_equal(tight.room_h, env["bbox_h"]) and tight.words < cs.words
    assert torch.equal(tight.to_planes(), env["planes"])
    assert tight.tighten(env["bbox_h"]) is tight


# --------------------------------------------------------------------------------------------------------------- tables
def _labels(n, seed):
    g = np.random.default_rng(seed)
    scores = (g.permutation(n) / n * 0.7 + 0.3).tolist()
    return scores, g.integers(0, 2, n).tolist(), np.sort(g.integers(0, 5, n)).tolist()


def test_to_table_equals_the_instance_table_of_the_planes(ops, env):
    from deepemia_amd import parallel
    scores, classes, units = _labels(env["n"], 64)
    hdr, pay = env["cs"].to_table(scores, classes, units)
    ref_hdr, ref_pay = parallel.encode_instance_table(env["planes"], scores, classes, units, env["bbox_h"], env["area_h"])
    assert hdr.dtype == ref_hdr.dtype and pay.dtype == ref_pay.dtype and pay.numel() > 1000
    assert torch.equal(hdr, ref_hdr) and torch.equal(pay, ref_pay)
    empty = env["cs"].select([])
    hdr0, pay0 = empty.to_table([], [], [])
    assert tuple(hdr0.shape) == (0, parallel.HDR) and pay0.numel() == 0


def test_from_table_of_a_gathered_buffer_equals_the_decoded_planes(ops, env):
    """A ``GlobalTable`` as ``all_gather_instance_tables`` returns it for two ranks, made by hand: each rank's slot = three slot words,
    its header rows up to the reserved capacity, its payload up to the reserved capacity (the slack holds a pattern no mask has);
    the merged header ordered by unit id (the ranks' units interleave), ``offsets`` pointing into the buffer."""
    from deepemia_amd import parallel
    from deepemia_amd.cropset import CropMaskSet
    n, dev = env["n"], ops.device
    scores, classes, _ = _labels(n, 65)
    halves = [np.arange(0, n, 2), np.arange(1, n, 2)]
    tables = []
    for r, idx in enumerate(halves):
        units = (2 * (np.arange(len(idx)) // 4) + r).tolist()                    # rank 0: units 0, 2, 4 ...; rank 1: 1, 3, 5 ...
        hdr, pay = env["cs"].select(idx).to_table([scores[i] for i in idx], [classes[i] for i in idx], units)
        hdr = hdr.cpu().numpy()
        if r == 0:                                                                # the N4 marker row of class 1: unit -1, no words
            mark = np.zeros((1, parallel.HDR), np.int32)
            mark[0, 0], mark[0, 1], mark[0, 4:8] = -1, 1, -1
            hdr = np.concatenate([mark, hdr])
        tables.append((hdr, pay.cpu().numpy()))
    S = parallel.SLOT_WORDS
    cn, cp = max(len(h) for h, _ in tables) + 5, max(len(p) for _, p in tables) + 777
    slot = S + cn * parallel.HDR + cp
    buf = np.full((2, slot), 0x5A5A5A5A, np.int32)
    hn, offs = [], []
    for r, (hdr, pay) in enumerate(tables):
        buf[r, :S] = [len(hdr), len(pay), 0]
        buf[r, S:S + hdr.size] = hdr.ravel()
        buf[r, S + cn * parallel.HDR:S + cn * parallel.HDR + len(pay)] = pay
        hn.append(hdr)
        offs.append(parallel._offsets(parallel._payload_lengths(hdr)) + (r * slot + S + cn * parallel.HDR))
    hn, offs = np.concatenate(hn), np.concatenate(offs)
    order = np.argsort(hn[:, 0], kind="stable")
    hn, offs = np.ascontiguousarray(hn[order]), offs[order]
    assert hn[0, 0] == -1 and not np.array_equal(order, np.arange(len(order))) and np.any(np.diff(offs) < 0)
    gt = parallel.GlobalTable(torch.from_numpy(hn).to(dev), torch.from_numpy(buf.ravel()).to(dev), hn, offs, np.zeros(2, np.int64))
    ref = parallel.decode_instance_table(gt.header, gt.payload, H, W, dev, host_header=gt.host_header, offsets=gt.offsets)[0]
    src_of_row = np.concatenate([[-1], halves[0], halves[1]])[order]            # which mask of env a row carries (-1: the marker)
    assert torch.equal(ref[1:], env["planes"][torch.from_numpy(src_of_row[1:]).to(dev)]) and int(ref[0].abs().sum()) == 0
    cs = CropMaskSet.from_table(ops, (H, W), gt.host_header, gt.payload, offsets=gt.offsets)
    assert len(cs) == len(hn) and torch.equal(cs.to_planes(), ref)
    assert np.array_equal(cs.room_h, hn[:, 4:8]) and np.array_equal(cs.bbox.cpu().numpy(), hn[:, 4:8]) and np.array_equal(cs.area.cpu().numpy(), hn[:, 8])
    # a class-major subset of the rows, the table's order kept inside a class; the marker is in neither
    rows = np.concatenate([np.nonzero((hn[:, 1] == c) & (hn[:, 0] != -1))[0] for c in (1, 0)])
    sub = CropMaskSet.from_table(ops, (H, W), gt.host_header, gt.payload, offsets=gt.offsets, rows=rows)
    assert len(sub) == len(rows) == n and torch.equal(sub.to_planes(), ref[torch.from_numpy(rows).to(dev)])
    assert np.array_equal(sub.area.cpu().numpy(), hn[rows, 8])
    # one rank's own table: words back to back in header order
    hdr0, pay0 = tables[1]
    own = CropMaskSet.from_table(ops, (H, W), hdr0, torch.from_numpy(pay0).to(dev))
    assert torch.equal(own.to_planes(), env["planes"][torch.from_numpy(halves[1]).to(dev)])
    assert len(CropMaskSet.from_table(ops, (H, W), hn, gt.payload, offsets=gt.offsets, rows=np.zeros(0, np.int64))) == 0


# --------------------------------------------------------------------------------------------------------------- memory
def test_the_exchange_of_a_crop_set_stays_far_below_the_decoded_planes(gpu_device):
    """400 masks (boxes <= 40 px) on a 1024^2 frame through to_table -> all_gather_instance_tables -> from_table in one process.  The
    plane exchange's decode alone allocates P = 400 x 1024 x 32 x 4 bytes = 50 MiB of zeroed planes; the crop form holds a handful
    of copies of <= 480 bytes per mask.  Bound: a quarter of P (measured on an MI355X: 152 576 bytes)."""
    from deepemia_amd import parallel
    from deepemia_amd.cropset import CropMaskSet, rooms_of_placed_tiles
    from deepemia_amd.maskset import MaskOps
    ops = MaskOps(gpu_device)
    h = w = 1024
    tile, n = 256, 400
    src = _blob_planes(ops, n, tile, tile, 41, max_box=40, dup=False)
    ops.set_frame_width(tile)
    _, sbb = ops.area_bbox(src)
    g = np.random.default_rng(42)
    xo, yo = (g.integers(0, 5, n) * 192).tolist(), (g.integers(0, 5, n) * 192).tolist()
    rooms = rooms_of_placed_tiles(sbb.cpu().numpy(), (tile, tile), (tile, tile), xo, yo, (h, w))
    assert (rooms[:, 0] >= 0).all()
    rooms[:, :2] = np.maximum(rooms[:, :2] - 3, 0)                                # rooms a little wider than the boxes: to_table tightens them
    rooms[:, 2:] = np.minimum(rooms[:, 2:] + 3, h - 1)
    ops.set_frame_width(w)
    placed = CropMaskSet.place_tiles(ops, src, rooms, xo, yo, tile, tile, h, w, src_w=tile)
    scores, classes, units = _labels(n, 43)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    hdr, pay = placed.to_table(scores, classes, units)
    gt = parallel.all_gather_instance_tables(hdr, pay)
    back = CropMaskSet.from_table(ops, (h, w), gt.host_header, gt.payload, offsets=gt.offsets)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    P = n * h * (w // 32) * 4
    print(f"to_table -> exchange -> from_table of {n} masks allocated {peak} bytes at most ({peak / 2**20:.2f} MiB); the decoded planes are {P / 2**20:.0f} MiB")
    assert np.array_equal(gt.host_header[:, 0], np.asarray(units)) and np.array_equal(back.room_h, placed.bbox.cpu().numpy())
    assert torch.equal(back.to_planes(), placed.to_planes()) and int(back.area.sum()) > 10000
    assert peak < P / 4


# ------------------------------------------------------------------------------------------- gather_and_merge, one process
def _fake_pipe(dev, settings):
    from deepemia_amd.functions.inference import InferencePipeline
    return InferencePipeline([types.SimpleNamespace(engine=types.SimpleNamespace(device=torch.device(dev)))], "t", dict(settings), {})


FORMS = {"planes": {"mask_frame": "full"}, "crops": {"mask_frame": "crop_direct", "rank_exchange": "crops"}}
H4 = W4 = 512
TILE4 = 128


def _placed(pipe, n, seed):
    """n masks on the 512^2 frame, every blob twice at the same place (the merge removes some): planes or a crop set."""
    from deepemia_amd.cropset import CropMaskSet, rooms_of_placed_tiles
    half = _blob_planes(pipe.ops, n // 2, TILE4, TILE4, seed, max_box=40, dup=False)
    src = torch.cat([half, half]).contiguous()
    pipe.ops.set_frame_width(TILE4)
    _, sbb = pipe.ops.area_bbox(src)
    g = np.random.default_rng(seed + 1)
    xo, yo = 2 * (g.integers(0, 5, n // 2) * 96).tolist(), 2 * (g.integers(0, 5, n // 2) * 96).tolist()
    pipe.ops.set_frame_width(W4)
    if not pipe.crop:
        return pipe.ops.place_tiles(src, xo, yo, TILE4, TILE4, H4, W4, src_w=TILE4)
    return CropMaskSet.place_tiles(pipe.ops, src, rooms_of_placed_tiles(sbb.cpu().numpy(), (TILE4, TILE4), (TILE4, TILE4), xo, yo, (H4, W4)), xo, yo,
                                   TILE4, TILE4, H4, W4, src_w=TILE4)


def _part(pipe, placed, lo, hi):
    return placed.select(np.arange(lo, hi)) if pipe.crop else placed[lo:hi].contiguous()


def _class_local(pipe, cls, n, seed, f32_scores, full="masks", tiles=True):
    """(full masks, scores, classes, [tile masks], scores, classes, units) of one class: a full-image part of n // 4 masks and two
    tile parts of units that interleave with the other classes' after the exchange's sort by unit id."""
    placed = _placed(pipe, n, seed)
    g = np.random.default_rng(seed + 2)
    sc = (g.permutation(n) / n * 0.6 + 0.3)
    sc = [np.float32(v) for v in sc] if f32_scores else [float(v) for v in sc]
    k, m = n // 4, n // 4 + (n - n // 4) // 2
    fm, fs, fc = (_part(pipe, placed, 0, k), sc[:k], [cls] * k) if full == "masks" else (full, [], [])
    if not tiles:
        return fm, fs, fc, [], [], [], []
    return fm, fs, fc, [_part(pipe, placed, k, m), _part(pipe, placed, m, n)], sc[k:], [cls] * (n - k), [1 + cls] * (m - k) + [3 + cls] * (n - m)


def _locals(pipe, n, classes=(0, 1, 2, 3, 4, 5)):
    made = {0: lambda: _class_local(pipe, 0, n, 100 + n, True),
            1: lambda: _class_local(pipe, 1, n, 200 + n, True),
            2: lambda: _class_local(pipe, 2, n, 300 + n, False, full="EMPTY_NDARRAY"),                  # N4 with tile masks: raises
            3: lambda: _class_local(pipe, 3, n, 400 + n, False, full="EMPTY_NDARRAY", tiles=False),     # N4 without: nothing
            4: lambda: (None, [], [], [], [], [], []),                                                    # a class with nothing
            5: lambda: _class_local(pipe, 5, n, 500 + n, False)}                                          # an ensemble's f64 scores
    return {c: made[c]() for c in classes}, {2: True, 3: True, 5: True}


def test_gather_and_merge_in_both_forms_one_process(gpu_device):
    from deepemia_amd.cropset import CropMaskSet
    from deepemia_amd.functions.inference import EmptyEnsembleTypeError
    pipes = {f: _fake_pipe(gpu_device, s) for f, s in FORMS.items()}
    waits = {}
    for f, pipe in pipes.items():
        pipe.begin_image_stats()
    for n in (20, 60):
        res = {}
        for f, pipe in pipes.items():
            loc, ens = _locals(pipe, n)
            w0 = pipe.d2h_waits
            res[f] = pipe.gather_and_merge(loc, (H4, W4), ens)
            waits[f, n] = pipe.d2h_waits - w0
        assert list(res["crops"]) == list(res["planes"]) == [0, 1, 2, 3, 4, 5]
        for cls in (0, 1, 5):
            (mp_, sp, cp), (mc, sc, cc) = res["planes"][cls], res["crops"][cls]
            assert 0 < len(sp) < n and isinstance(mc, CropMaskSet) and torch.equal(mc.to_planes(), mp_)
            assert sc == sp and [type(v) for v in sc] == [type(v) for v in sp] and cc == cp == [cls] * len(sp)
            assert type(sp[0]) is (float if cls == 5 else np.float32)
        for f in FORMS:
            assert type(res[f][2]) is EmptyEnsembleTypeError
            assert res[f][3] == (None, [], []) and res[f][4] == (None, [], [])
    # the crop form's waits: the tables' boxes, the exchange, the merge -- whatever the instance and class count
    pipe = pipes["crops"]
    for classes in ((0,), (0, 1)):
        loc, ens = _locals(pipe, 20, classes)
        w0 = pipe.d2h_waits
        pipe.gather_and_merge(loc, (H4, W4), ens)
        waits["crops", classes] = pipe.d2h_waits - w0
    assert waits["crops", 20] == waits["crops", 60] == waits["crops", (0,)] == waits["crops", (0, 1)] == 3
    st = pipe.end_image_stats((H4, W4))
    assert st["full_frame_planes_peak"] == 0 and st["plane_pool_capacity"] == 0
    assert pipes["planes"].end_image_stats((H4, W4))["full_frame_planes_peak"] > 0


def test_a_failing_crop_table_still_takes_part_in_the_exchange(gpu_device, monkeypatch):
    from deepemia_amd import parallel
    from deepemia_amd.functions.inference import PeerImageFailure
    pipe = _fake_pipe(gpu_device, FORMS["crops"])
    loc, ens = _locals(pipe, 20, (0, 1))
    seen = []
    orig = parallel.all_gather_instance_tables

    def recording(header, payload, **kw):
        seen.append((int(header.shape[0]), int(payload.shape[0]), kw.get("status")))
        return orig(header, payload, **kw)

    def failing(*a, **k):
        raise RuntimeError("injected failure of the crop table")

    monkeypatch.setattr(parallel, "all_gather_instance_tables", recording)
    pipe._crop_table = failing
    with pytest.raises(PeerImageFailure, match="every rank skips this image"):
        pipe.gather_and_merge(loc, (H4, W4), ens)
    assert seen == [(0, 0, 1)]                                                   # an empty table with status 1 went through the exchange
    del pipe._crop_table
    out = pipe.gather_and_merge(loc, (H4, W4), ens)
    assert seen[-1][0] == 40 and seen[-1][2] == 0 and len(out[0][1]) > 0


# ------------------------------------------------------------------------------------------------------------- two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run_tile_pipeline(settings):
    from deepemia_amd import synth
    from deepemia_amd.engine import MaskRCNNEngine
    from deepemia_amd.functions.inference import InferencePipeline
    from deepemia_amd.predictor import Predictor

    sd = synth.random_d2_state_dict(50, 2, seed=0, mask_bias=0.5, mask_gain=6.0)
    pipe = InferencePipeline([Predictor(MaskRCNNEngine(sd, 50, 2, 0.3, "cuda:0", "f32"))], "t", dict(settings), {})
    img = torch.from_numpy(synth.em_tile(77, 1024)).to("cuda:0")
    pipe.begin_image_stats()
    res = []
    for cls, conf, thr in ((0, 0.3, 0.6), (1, 0.35, 0.5)):
        m, s, c = pipe.tile_based_inference_pipeline([0], "img", img, cls, {1}, conf, 512, 0.25, 1.0, thr, True)
        if m is not None:
            m = (m.to_planes() if pipe.crop else m).cpu().numpy()
        res.append((m, [float(v) for v in s], list(c)))
    return res, pipe.forward_calls, pipe.end_image_stats((1024, 1024))["full_frame_planes_peak"]


def _sharded_worker(rank, world, port, tmp, out):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), DEEPEMIA_LOG_DIR=str(tmp))
    dist.init_process_group("gloo", rank=rank, world_size=world)   # both ranks share the one GPU of the test box
    out[rank] = _run_tile_pipeline(FORMS["crops"])
    dist.barrier()
    dist.destroy_process_group()


def test_tiles_sharded_over_two_ranks_with_crops_equal_the_single_process_planes(gpu_device, tmp_path):
    import torch.multiprocessing as mp

    single, calls1, planes1 = _run_tile_pipeline(FORMS["planes"])
    out = mp.Manager().dict()
    mp.spawn(_sharded_worker, args=(2, _free_port(), tmp_path, out), nprocs=2, join=True)
    for r in range(2):
        res, calls, planes_peak = out[r]
        for (ma, sa, ca), (mb, sb, cb) in zip(res, single):
            assert (ma is None) == (mb is None)
            if ma is not None:
                np.testing.assert_array_equal(ma, mb)
            assert sa == sb and ca == cb
        assert planes_peak == 0
    assert out[1][1] < calls1 and planes1 > 0          # rank 1 ran fewer forwards (no full-image pass, half the tiles)
    assert sum(len(x[1]) for x in single) > 20


# ------------------------------------------------------------------------------------------------------------------ CLI
CLI_ARGS = ["--task", "inference", "--dataset_name", DATASET, "--threshold", "0.3", "--no-gpu-check"]


def _cli_rank_worker(rank, world, port, root, cfgdir, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      DEEPEMIA_DIST_BACKEND="gloo", DEEPEMIA_CONFIG_DIR=str(cfgdir), DEEPEMIA_OFFLINE="1", DEEPEMIA_LOG_DIR=str(root),
                      DEEPEMIA_SHARD="tiles", DEEPEMIA_ONE_DEVICE="1", DEEPEMIA_WORKERS="1")
    os.chdir(root)
    import main as cli
    from deepemia_amd.functions import inference as inf_mod

    rc = cli.main(CLI_ARGS)
    out[rank] = (rc, dict(inf_mod.LAST_RUN_STATS))


def test_cli_two_ranks_with_crops_write_the_one_process_bytes(tmp_path, monkeypatch, gpu_device):
    import main as cli
    import torch.multiprocessing as mp
    from deepemia_amd.utils import config as C

    ds_cfg = {"inference_overrides": {"confidence_mode": "manual",
                                      "class_specific_settings": {"class_0": {"confidence_threshold": 0.3, "iou_threshold": 0.6},
                                                                  "class_1": {"confidence_threshold": 0.35, "iou_threshold": 0.5}},
                                      "tile_settings": {"tile_size": 200, "overlap_ratio": 0.125, "upscale_factor": 1.0, "edge_filter_enabled": True},
                                      "spatial_constraints": {"enabled": True, "containment_rules": {1: 0}, "containment_threshold": 0.5}}}
    cfgdir, split = _write_tree(tmp_path, ds_cfg)

    def settings(extra):
        cfg = json.loads(json.dumps(ds_cfg))
        cfg["inference_overrides"].update(extra)
        (cfgdir / "datasets" / f"{DATASET}.yaml").write_text(yaml.safe_dump(cfg, sort_keys=False))

    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(cfgdir))
    monkeypatch.setenv("DEEPEMIA_OFFLINE", "1")
    monkeypatch.setenv("DEEPEMIA_WORKERS", "1")
    monkeypatch.chdir(tmp_path)
    names = ["measurements_results.csv", "R50_flip_results.csv", "class_color_legend.txt"]
    settings(FORMS["planes"])
    C.reset_cache()
    assert cli.main(CLI_ARGS) == 0
    C.reset_cache()
    single = {nm: (split / nm).read_bytes() for nm in names}
    for nm in names:
        (split / nm).unlink()
    assert len(single["measurements_results.csv"].splitlines()) > 10 and len(single["R50_flip_results.csv"].splitlines()) > 10
    settings(FORMS["crops"])
    out = mp.Manager().dict()
    mp.spawn(_cli_rank_worker, args=(2, _free_port(), str(tmp_path), str(cfgdir), out), nprocs=2, join=True)
    assert {r: v[0] for r, v in out.items()} == {0: 0, 1: 0}
    for nm in names:
        assert (split / nm).read_bytes() == single[nm], nm
    for r in range(2):
        assert out[r][1]["mask_frame"] == "crop_direct" and out[r][1]["full_frame_planes_peak"] == 0
