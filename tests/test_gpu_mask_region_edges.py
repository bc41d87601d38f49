"""GPU: the per-mask region stages of ``csrc/maskregion.h`` at the edges of their STRUCTURE -- variant boundaries, regions wider
than 64 words, band partitions, frame edges, hints, stage programs, both ways of counting components and the flood's round
limit -- bit for bit against the scipy-backed ``oracle/postproc_ref.py`` (``fill_holes``, ``erode_cross``, ``dilate_cross``,
``n_components8``, ``find_external_contours``).  The cases and what each of them reaches are in ``tests/mask_region_cases.py``;
``test_cpu_mask_region_cases.py`` shows on the CPU that they sit where their names say and that the reference notices each
structural fault they are there for.  No tolerances: planes, areas, boxes and flags are exact.

One test per family; the cases of a family that share a frame, a program and a gate go through ONE call, so the worklist sees
small, large and HBM-sized regions side by side.

H, seen on an MI355X with the round limit ``2 * (rh + 32 * rw) + 8`` the flood had before these tests: `fill` closed the end of
the channel of the 64 x 500, the 130 x 2040 and the 20 x 2080 serpentine (lockstep model: 1744, 7643, 6235 rounds against
limits of 1164, 4368, 4276); the 30 x 250 control (434 of 584, 4 waves) and the serpentine with horizontal legs passed, and so
did every component flag (the walls hang from one row: a short flood).  With the proven limit ``32 * rh * rw + 1`` all pass.
"""
import numpy as np
import pytest
import torch

import mask_region_cases as M

pytestmark = pytest.mark.gpu

_REF = {}


@pytest.fixture(scope="module")
def ops(gpu_device):
    from deepemia_amd.maskset import MaskOps

    return MaskOps(gpu_device)


def expected(c):
    """(mask, flag) of the case's program from the oracle, computed once per (mask, program, gate)."""
    from oracle import postproc_ref as P

    key = (id(c.mask), c.program, c.active)
    if key not in _REF:
        _REF[key] = M.run_program_ref(c.mask, c.program, c.active, P)
    return _REF[key]


def run_batch(ops, cs, hint):
    """One ``program_`` call over the cases (same frame, program and gate); returns what differs from the oracle."""
    c0 = cs[0]
    H, W, n = c0.H, c0.W, len(cs)
    boxes = np.asarray([M.hint_box(c.mask, hint) for c in cs], dtype=np.int32)
    fails = []
    ops.set_frame_width(W)
    try:
        p = ops.from_dense(np.stack([c.mask for c in cs]))
        active = None if c0.active is None else torch.full((n,), c0.active, dtype=torch.uint8, device=ops.device)
        area, bb, flag = ops.program_(p, list(c0.program), torch.from_numpy(boxes).to(ops.device), active)
        got = ops.to_dense(p, W)
        area, bb, flag = area.cpu().numpy(), bb.cpu().numpy(), flag.cpu().numpy()
        if W % 32:
            assert int((p[:, :, -1] >> (W % 32)).abs().sum()) == 0, (c0.name, hint, "padding bits set")
    finally:
        ops.set_frame_width(0)
    for i, c in enumerate(cs):
        want, wflag = expected(c)
        what = []
        if not np.array_equal(got[i], want):
            what.append(f"{int((got[i] != want).sum())} pixels differ")
        if int(area[i]) != int(want.sum()):
            what.append(f"area {int(area[i])} != {int(want.sum())}")
        if tuple(int(v) for v in bb[i]) != M.tight_box(want):
            what.append(f"bbox {bb[i].tolist()} != {M.tight_box(want)}")
        if int(flag[i]) != wflag:
            what.append(f"flag {int(flag[i])} != {wflag}")
        if what:
            fails.append(f"{c.name} [{hint} hint]: " + ", ".join(what))
    return fails


def run_family(ops, cs, hints=M.HINTS):
    fails = []
    for batch in M.batches(cs):
        for hint in hints:
            fails += run_batch(ops, batch, hint)
    return fails


def check_contours(ops, masks, max_contours=64):
    from oracle import postproc_ref as P

    W = masks.shape[2]
    ops.set_frame_width(W)
    try:
        recs = ops.trace(ops.from_dense(masks), max_contours=max_contours).records(measure=False)
    finally:
        ops.set_frame_width(0)
    for i, m in enumerate(masks):
        ref = P.find_external_contours(m)
        assert len(ref) == len(recs[i]) <= max_contours, (i, len(ref), len(recs[i]))
        for rec, c in zip(recs[i], ref):
            np.testing.assert_array_equal(rec["points"], c, err_msg=f"mask {i}")


def test_a_variant_boundaries_and_both_entries(ops):
    """Regions of exactly 1024 / 1056 and 8192 / 8256 words under two programs; then one batch of a small, a large, an HBM-sized
    and an empty mask through ``demia_mask_program_wl`` and ``demia_mask_program``: identical planes, areas, boxes and flags."""
    from deepemia_amd import _lib

    fails = run_family(ops, M.cases("A"))
    assert not fails, "\n".join(fails)
    cs, prog = M.mixed_batch()
    H, W, n = cs[0].H, cs[0].W, len(cs)
    code = sum(_lib.MOP[s] << (4 * i) for i, s in enumerate(prog))
    boxes = torch.from_numpy(np.asarray([M.hint_box(c.mask, "tight") for c in cs], dtype=np.int32)).to(ops.device)
    stream = int(torch.cuda.current_stream(ops.device).cuda_stream)
    res = []
    for with_list in (True, False):
        p = ops.from_dense(np.stack([c.mask for c in cs]))
        scratch = torch.empty_like(p)
        area = torch.full((n,), -7, dtype=torch.int32, device=ops.device)
        bb = torch.full((n, 4), -7, dtype=torch.int32, device=ops.device)
        flag = torch.full((n,), -7, dtype=torch.int32, device=ops.device)
        if with_list:
            wl = torch.full((n + 2,), -7, dtype=torch.int32, device=ops.device)
            st = ops.lib.demia_mask_program_wl(_lib.ptr(p), _lib.ptr(scratch), _lib.ptr(boxes), 0, code, n, H, W, _lib.ptr(area), _lib.ptr(bb),
                                               _lib.ptr(flag), _lib.ptr(wl), stream)
        else:
            st = ops.lib.demia_mask_program(_lib.ptr(p), _lib.ptr(scratch), _lib.ptr(boxes), 0, code, n, H, W, _lib.ptr(area), _lib.ptr(bb),
                                            _lib.ptr(flag), stream)
        _lib.check(st, "demia_mask_program")
        torch.cuda.synchronize(ops.device)
        if with_list:
            assert int(wl[0]) == 2 and sorted(wl[2:4].tolist()) == [1, 2]                   # the large and the HBM-sized mask, listed once each
        res.append((p, area, bb, flag))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    p, area, bb, flag = res[0]
    got = ops.to_dense(p, W)
    for i, c in enumerate(cs):
        want, wflag = expected(c)
        np.testing.assert_array_equal(got[i], want, err_msg=c.name)
        assert int(area[i]) == int(want.sum()) and tuple(bb[i].tolist()) == M.tight_box(want) and int(flag[i]) == wflag, c.name


def test_b_regions_wider_than_64_words(ops):
    """rw 65, 66, 129, 130 at word column 3, in LDS and in HBM: holes, channels and diagonal links across region words 63|64
    and 127|128; the masks of two of them also through the contour tracer."""
    fails = run_family(ops, M.cases("B"))
    assert not fails, "\n".join(fails[:40])
    pick = [c.mask for c in M.cases("B") if c.program == ("fill",) and ("rw66_" in c.name or "rw129_large" in c.name)]
    assert len(pick) == 6
    check_contours(ops, np.stack(pick))


def test_c_band_partitions(ops):
    """1 to 17 region rows with 4 waves and, from 3 rows on, with 8 (regions up to 342 words wide): rings and 1-px vertical
    channels across every band, waves without a band, frames of one and two rows."""
    fails = run_family(ops, M.cases("C"))
    assert not fails, "\n".join(fails[:40])


def test_d_frame_edges(ops):
    """Frames 1 .. 65 wide and 1 .. 40 high: full frame, border, ring inside the border, corners, cavities open to a frame edge;
    fill, erode, dilate, closing, component test, area / box and the padding bits, by stage program and by the single calls."""
    from oracle import postproc_ref as P

    fails = run_family(ops, M.cases("D"))
    assert not fails, "\n".join(fails[:40])
    frames = {}
    for c in M.cases("D"):
        frames.setdefault((c.H, c.W), {})[id(c.mask)] = c.mask
    for (H, W), ms in frames.items():
        masks = np.stack(list(ms.values()))
        ops.set_frame_width(W)
        try:
            p = ops.from_dense(masks)
            np.testing.assert_array_equal(ops.to_dense(p, W), masks)
            fill, er, di = ops.fill_holes(p), ops.erode(p), ops.dilate(p)
            flags = ops.components_gt1(p).cpu().numpy()
            area, bbox = ops.area_bbox(p)
            a2, b2 = ops.area_bbox(p, bbox)
            assert torch.equal(area, a2) and torch.equal(bbox, b2)
            for t in (fill, er, di):
                assert W % 32 == 0 or int((t[:, :, -1] >> (W % 32)).abs().sum()) == 0
            fill, er, di = ops.to_dense(fill, W), ops.to_dense(er, W), ops.to_dense(di, W)
            for i, m in enumerate(masks):
                tag = f"{H}x{W} mask {i}"
                np.testing.assert_array_equal(fill[i], P.fill_holes(m), err_msg=tag)
                np.testing.assert_array_equal(er[i], P.erode_cross(m), err_msg=tag)
                np.testing.assert_array_equal(di[i], P.dilate_cross(m), err_msg=tag)
                assert int(flags[i]) == int(P.n_components8(m) > 1), tag
                assert int(area[i]) == int(m.sum()) and tuple(bbox[i].tolist()) == M.tight_box(m), tag
        finally:
            ops.set_frame_width(0)


def test_f_stage_programs(ops):
    """Eight slots and four dilations clipped at a frame corner, a flag OR-ed over two flag stages, the gate without an ``active``
    array, closed and open, stages after a drop that emptied the mask."""
    fails = run_family(ops, M.cases("F"))
    assert not fails, "\n".join(fails[:40])


def test_g_component_count_by_euler_number_and_by_flood(ops):
    fails = run_family(ops, M.cases("G"))
    assert not fails, "\n".join(fails[:40])


def test_h_flood_round_limit_on_serpentines(ops):
    """1-px serpentine channels: the background flood needs about (legs x bands) rounds.  scipy: nothing to fill, one component."""
    cs = M.cases("H")
    for c in cs:
        want, wflag = expected(c)
        assert np.array_equal(want, c.mask) and wflag == 0, c.name
    fails = run_family(ops, cs, hints=("tight",))
    for c in cs:
        print(f"{c.name}: {'FAILED' if any(f.startswith(c.name + ' ') for f in fails) else 'ok'}")
    assert not fails, "\n".join(fails)
    check_contours(ops, np.stack([c.mask for c in cs if c.name in ("H_64x500_lds8_fill", "H_30x250_control_fill")]), max_contours=8)
