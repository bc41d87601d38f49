"""``demia_paste_masks``, ``demia_unpack_masks`` and ``demia_mask_area_bbox`` (csrc/paste.hip) at edge geometry, against an
independent f64 reference, through the C ABI the way ``engine.paste``, ``engine.unpack`` and ``engine.area_bbox`` call it.

The calls are the table of ``paste_cases.py`` (frames 32 to 2300 px wide, both column paths of the kernel and the windows of
exactly 2048 and 2049 columns between them, rescaling by unequal non-dyadic ratios, boxes outside the frame, clipped to
nothing, under a pixel wide, inside and across words, counts of 0, 1 and D, an exact family); the reference is
``paste_ref.py`` (box contract in numpy f32, sampling in f64).  ``test_cpu_paste_ref.py`` checks table and reference without
a GPU.

What is exact: ``out_boxes`` (bit for bit), ``valid``, the hint (the reference window, or -1), zero planes for invalid and
unused slots, no bit outside the hint, no bit past W in a row's last word, and every pixel of the exact family.

The tie band.  Elsewhere a pixel has to equal the f64 decision ``p >= 0.5`` unless ``|p - 0.5| <= TAU`` = 2^-14 = 6.1e-5; the
number of mismatches outside the band must be 0.  Why 2^-14: where a tap is in range, the kernel's sampling coordinate
``ix = ((gx + 1) * 28 - 1) / 2`` with ``gx = (X + 0.5 - x0) / (x1 - x0) * 2 - 1`` is a chain of six f32 operations on values of
magnitude <= ~32, each with a relative error <= 2^-24 = 6e-8: ``ix`` and ``iy`` are each off by less than 6 * 32 * 6e-8 =
1.2e-5 in the worst case and typically by a few 1e-6.  The mask holds probabilities in [0, 1], so the bilinear surface has a
slope <= 1 per cell in each direction (and is continuous across cells and into the zero padding, so a coordinate that lands
in the neighbouring cell changes nothing more): the two coordinate errors move p by less than 2.4e-5.  The four products
and three sums of the interpolation add about 1e-7.  That bounds |p32 - p64| by 2.5e-5 < TAU / 2; the CPU oracle's f32 path,
the same formula in another order, is within 4.6e-6 of the reference over this table (printed and bounded by
``test_cpu_paste_ref.py``).  A kernel that needs more than TAU on a pixel has a fault to be explained, not a band to be widened.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import paste_cases as T
import paste_ref as REF

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A        # what the plane buffer holds before a whole-plane paste: every word has to be overwritten
GUARD = 1024                 # words behind the planes that no paste may touch


@pytest.fixture(scope="module")
def gpu(gpu_device):
    from deepemia_amd import _lib

    return dict(dev=gpu_device, lib=_lib.load(), L=_lib)


def _stream(g) -> int:
    return int(torch.cuda.current_stream(g["dev"]).cuda_stream)


def new_planes(g, case, fill):
    f = case.frame
    n = case.N * case.D * f.out_h * f.wpr
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.int32, device=g["dev"])
    buf[:n] = fill
    return buf


def run_paste(g, case, buf=None, prev=None):
    """One ``demia_paste_masks`` call of the case.  ``buf``: the plane buffer (with its guard) to paste into -- a fresh one
    full of the sentinel when None; ``prev``: the previous boxes of an incremental paste."""
    L, lib, dev, f = g["L"], g["lib"], g["dev"], case.frame
    N, D = case.N, case.D
    mp = torch.from_numpy(case.mask_prob()).to(dev)
    assert mp.shape == (N * D * 196 * 4, (case.K + 3) // 4 * 4)
    boxes = torch.from_numpy(case.det_boxes()).to(dev)
    classes = torch.from_numpy(case.classes()).to(dev)
    cnt = torch.tensor(case.counts, dtype=torch.int32, device=dev)
    ob = torch.full((N, D, 4), float("nan"), dtype=torch.float32, device=dev)
    valid = torch.full((N, D), 9, dtype=torch.uint8, device=dev)
    bbox = torch.full((N, D, 4), -7, dtype=torch.int32, device=dev)
    if buf is None:
        buf = new_planes(g, case, SENTINEL)
    nwords = N * D * f.out_h * f.wpr
    assert buf.numel() == nwords + GUARD and boxes.shape == (N, D, 4) and classes.shape == (N, D)
    d = L.PasteDesc(L.ptr(mp), mp.shape[-1], L.ptr(boxes), L.ptr(classes), L.ptr(cnt), N, D, f.img_h, f.img_w, f.out_h, f.out_w,
                    L.ptr(ob), L.ptr(valid), L.ptr(buf), L.ptr(bbox), L.ptr(prev))
    L.check(lib.demia_paste_masks(C.byref(d), _stream(g)), "demia_paste_masks")
    torch.cuda.synchronize()
    host = buf.cpu().numpy().view(np.uint32)
    assert (host[nwords:] == SENTINEL).all(), (case.name, "the guard behind the planes was written")
    return dict(ob=ob.cpu().numpy(), valid=valid.cpu().numpy(), hint=bbox.cpu().numpy(), hint_dev=bbox,
                words=host[:nwords].reshape(N, D, f.out_h, f.wpr), buf=buf)


def check_case(case, out, what):
    """Everything a paste of the case has to leave behind; returns the list of what differs."""
    ref, f = T.reference(case), case.frame
    H, W = f.out_h, f.out_w
    fails = []
    if not np.array_equal(out["ob"].view(np.uint32), ref.out_boxes.view(np.uint32)):
        bad = np.argwhere((out["ob"].view(np.uint32) != ref.out_boxes.view(np.uint32)).any(axis=2))
        fails.append(f"out_boxes differ at {[(int(n), case.slots[n][i].name) for n, i in bad[:5]]}")
    if not np.array_equal(out["valid"], ref.valid.astype(np.uint8)):
        bad = np.argwhere(out["valid"] != ref.valid.astype(np.uint8))
        fails.append(f"valid differs at {[(int(n), case.slots[n][i].name, int(out['valid'][n, i])) for n, i in bad[:5]]}")
    if not np.array_equal(out["hint"], ref.hint):
        bad = np.argwhere((out["hint"] != ref.hint).any(axis=2))
        fails.append(f"hint differs at {[(int(n), case.slots[n][i].name, out['hint'][n, i].tolist(), ref.hint[n, i].tolist()) for n, i in bad[:5]]}")
    bits = REF.unpack_bits(out["words"], W)
    if bits[..., W:].any():
        fails.append(f"{int(bits[..., W:].sum())} bits set past W in the last word of a row")
    dense = bits[..., :W]
    in_band = off_band = 0
    need = 0.0
    for n in range(case.N):
        for i in range(case.D):
            name = (n, i, case.slots[n][i].name)
            if not ref.valid[n, i]:
                if dense[n, i].any():
                    fails.append(f"{name}: {int(dense[n, i].sum())} pixels set in the plane of an invalid or unused slot")
                continue
            y0, x0, y1, x1 = (int(v) for v in ref.hint[n, i])
            got = dense[n, i, y0:y1 + 1, x0:x1 + 1]
            outside = int(dense[n, i].sum()) - int(got.sum())
            if outside:
                fails.append(f"{name}: {outside} pixels set outside the hint")
            p = ref.prob[(n, i)]
            wrong = got != (p >= 0.5)
            if wrong.any():
                dec = T.decided(case, p)
                in_band += int((wrong & ~dec).sum())
                need = max(need, float(np.abs(p - 0.5)[wrong].max()))
                k = int((wrong & dec).sum())
                if k:
                    off_band += k
                    yy, xx = np.argwhere(wrong & dec)[0]
                    fails.append(f"{name}: {k} pixels differ from the f64 decision outside the tie band, first at y {y0 + yy} x {x0 + xx} "
                                 f"with p = {p[yy, xx]!r} (box {ref.out_boxes[n, i].tolist()}, path {T.column_path(ref.hint[n, i])})")
    print(f"{what}: {int(ref.valid.sum())} valid slots, {off_band} mismatches outside the band, {in_band} inside it, "
          f"band needed {need:.3e} (TAU {0.0 if case.exact else T.TAU:.3e})")
    return fails


@pytest.mark.parametrize("name", [c.name for c in T.CASES])
def test_whole_plane_paste_on_the_case_table(gpu, name):
    case = T.BY_NAME[name]
    out = run_paste(gpu, case)
    assert not (out["words"] == SENTINEL).all(axis=(2, 3)).any(), "a plane was not written"
    fails = check_case(case, out, name)
    assert not fails, (name, len(fails), fails[:8])


@pytest.mark.parametrize("frame", list(T.INCREMENTAL))
def test_incremental_paste_of_three_table_cases_into_the_same_planes(gpu, frame):
    """What a captured forward does on every replay: the planes were zeroed once, ``prev_bbox`` holds the boxes the last paste
    could set, and only the new boxes and the previous ones are written.  Three cases of one frame in a row -- boxes that
    move, a round with every slot in use, a round in which almost every instance is gone or invalid -- each checked against
    the f64 reference (zeros everywhere else included), never against the whole-plane kernel."""
    cases = [T.BY_NAME[n] for n in T.INCREMENTAL[frame]]
    buf = new_planes(gpu, cases[0], 0)
    prev = torch.full((cases[0].N, cases[0].D, 4), -1, dtype=torch.int32, device=gpu["dev"])
    for rnd, case in enumerate(cases):
        before = prev.clone()
        out = run_paste(gpu, case, buf=buf, prev=prev)
        assert torch.equal(prev, before), (frame, rnd, "the paste wrote its prev_bbox")
        fails = check_case(case, out, f"incremental {frame} round {rnd} ({case.name})")
        assert not fails, (frame, rnd, case.name, len(fails), fails[:8])
        prev.copy_(out["hint_dev"])                          # as engine.paste does after an incremental call
        assert np.array_equal(prev.cpu().numpy(), T.reference(case).hint), (frame, rnd)


# ------------------------------------------------------------------------------------------------------------------
# the packed-mask utilities
# ------------------------------------------------------------------------------------------------------------------
def unpack(g, words: np.ndarray, H: int, W: int) -> np.ndarray:
    """``demia_unpack_masks`` of uint32 [M, H, wpr] -> bool [M, H, W]; every byte written with 0 or 1, none behind the end."""
    L, dev = g["L"], g["dev"]
    M = words.shape[0]
    p = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(dev)
    n, guard = M * H * W, 256
    out = torch.full((n + guard,), 0xAB, dtype=torch.uint8, device=dev)
    L.check(g["lib"].demia_unpack_masks(L.ptr(p), L.ptr(out), M, H, W, _stream(g)), "demia_unpack_masks")
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert (host[n:] == 0xAB).all(), "unpack wrote behind its output"
    assert (host[:n] <= 1).all(), "unpack left a byte unwritten or wrote something other than 0 / 1"
    return host[:n].reshape(M, H, W).astype(bool)


def area_bbox(g, words: np.ndarray, H: int, W: int, hint=None):
    L, dev = g["L"], g["dev"]
    M = words.shape[0]
    p = torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(dev)
    h = None if hint is None else torch.from_numpy(np.ascontiguousarray(hint, dtype=np.int32)).to(dev)
    area = torch.full((M,), -5, dtype=torch.int32, device=dev)
    bbox = torch.full((M, 4), -5, dtype=torch.int32, device=dev)
    L.check(g["lib"].demia_mask_area_bbox(L.ptr(p), L.ptr(h), L.ptr(area), L.ptr(bbox), M, H, W, _stream(g)), "demia_mask_area_bbox")
    torch.cuda.synchronize()
    return area.cpu().numpy(), bbox.cpu().numpy()


def numpy_area_bbox(dense):
    ab = [REF.tight_box(m) for m in dense]
    return np.array([a for a, _ in ab], dtype=np.int32), np.array([b for _, b in ab], dtype=np.int32).reshape(len(ab), 4)


@pytest.mark.parametrize("name", ["geom_w33", "geom_w77", "geom_w128", "geom_wide", "rand_w333", "exact_family"])
def test_unpack_and_area_bbox_on_pasted_planes(gpu, name):
    """The planes a paste leaves, through ``unpack`` and through ``area_bbox`` with the paste's own hints and without any:
    equal to numpy on the host-unpacked words; the paste's hint contains every set pixel, so both give the same."""
    case = T.BY_NAME[name]
    f = case.frame
    H, W = f.out_h, f.out_w
    out = run_paste(gpu, case)
    words = out["words"].reshape(-1, H, f.wpr)
    dense = REF.unpack_bits(words, W)[..., :W]
    assert dense.any()
    assert np.array_equal(unpack(gpu, words, H, W), dense)
    want_area, want_box = numpy_area_bbox(dense)
    for hint in (None, out["hint"].reshape(-1, 4)):
        area, box = area_bbox(gpu, words, H, W, hint)
        assert np.array_equal(area, want_area), (name, hint is None)
        assert np.array_equal(box, want_box), (name, hint is None)


def planted(H: int, W: int):
    """Named bool planes [H, W]: empty, single bits at the four corners and on both sides of every kind of word boundary,
    rows and columns at the frame's edge, random rectangles."""
    rng = np.random.default_rng(W)
    planes = {"empty": []}
    for nm, y, x in (("top_left", 0, 0), ("top_right", 0, W - 1), ("bottom_left", H - 1, 0), ("bottom_right", H - 1, W - 1)):
        planes[f"corner_{nm}"] = [(y, x)]
    planes["all_four_corners"] = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)]
    planes["bit_31_of_word_0"] = [(H // 2, 31)]
    if W > 32:
        planes["bit_0_of_word_1"] = [(H // 2, 32)]
        planes["bit_31_and_bit_0_across_the_boundary"] = [(H // 2, 31), (H // 2 + 1, 32)]
    last = 32 * ((W - 1) // 32)
    planes["first_bit_of_the_last_word"] = [(1, last)]
    if last:
        planes["last_bit_before_the_last_word"] = [(H - 2, last - 1)]
    out = {}
    for k, pts in planes.items():
        m = np.zeros((H, W), dtype=bool)
        for y, x in pts:
            m[y, x] = True
        out[k] = m
    for k in range(4):
        m = np.zeros((H, W), dtype=bool)
        y0, x0 = int(rng.integers(0, H - 3)), int(rng.integers(0, W - 3))
        y1, x1 = int(rng.integers(y0 + 1, H + 1)), int(rng.integers(x0 + 1, W + 1))
        m[y0:y1, x0:x1] = rng.random((y1 - y0, x1 - x0)) > (0.3 if k % 2 else 0.97)
        out[f"random_rectangle_{k}"] = m
    out["full"] = np.ones((H, W), dtype=bool)
    out["last_column"] = np.zeros((H, W), dtype=bool)
    out["last_column"][:, W - 1] = True
    out["last_row"] = np.zeros((H, W), dtype=bool)
    out["last_row"][H - 1, :] = True
    return out


@pytest.mark.parametrize("W", [33, 77, 128, 2300])
def test_unpack_and_area_bbox_on_planted_planes(gpu, W):
    """Planted planes through ``unpack`` (W % 32 != 0: the byte path with a partial last word; 128: the 16-byte path) and
    ``area_bbox`` without a hint and with hints that are tight, loose, reaching beyond the frame (the kernel clips them) and
    -1 (nothing is read: area 0, box -1) -- against numpy on the dense planes."""
    H = 21
    planes = planted(H, W)
    names = list(planes)
    dense = np.stack([planes[k] for k in names])
    words = REF.pack_bits(dense)
    assert words.shape == (len(names), H, (W + 31) // 32)
    assert np.array_equal(unpack(gpu, words, H, W), dense)
    want_area, want_box = numpy_area_bbox(dense)
    empty = want_area == 0
    tight = want_box
    loose = np.where(empty[:, None], -1, np.stack([np.maximum(tight[:, 0] - 5, 0), np.maximum(tight[:, 1] - 37, 0),
                                                   np.minimum(tight[:, 2] + 4, H - 1), np.minimum(tight[:, 3] + 33, W - 1)], axis=1))
    beyond = np.where(empty[:, None], -1, np.stack([np.maximum(tight[:, 0] - 2, 0), tight[:, 1] - 70, tight[:, 2] + 50, tight[:, 3] + 100], axis=1))
    for what, hint in (("none", None), ("tight", tight), ("loose", loose), ("beyond the frame", beyond)):
        if hint is not None:
            # what the kernel may index after its clip stays inside the plane: rows 0 .. H - 1 and words 0 .. wpr - 1
            h = hint[~empty]
            assert (h[:, 0] >= 0).all() and (h[:, 0] <= H - 1).all() and (h[:, 1] <= W - 1).all() and (h[:, 2] >= h[:, 0]).all() and (h[:, 3] >= 0).all()
        area, box = area_bbox(gpu, words, H, W, hint)
        bad = [names[i] for i in range(len(names)) if area[i] != want_area[i] or box[i].tolist() != want_box[i].tolist()]
        assert not bad, (W, what, bad)
    area, box = area_bbox(gpu, words, H, W, np.full((len(names), 4), -1, dtype=np.int32))
    assert not area.any() and (box == -1).all(), (W, "hint -1")
