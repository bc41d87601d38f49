"""Device-resident sets of bit-packed instance masks and the HIP operations on them.

Everything the reference does with dense ``(H, W)`` numpy masks after ``predictor(image)``
(hole filling, cross erosion / dilation, overlap removal, connected-component test, pair
intersection counts, tile placement, contour tracing and the measurement reductions) runs here on
``[M, H, W/32]`` int32 tensors through the C ABI.  Only small tables (areas, boxes, pair counts,
contour points, measurement rows) ever reach the host.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import partial
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import os
import numpy as np
import torch

from . import _lib


# (A/B switch) 0: the large-region variants of the per-mask kernels run over all masks again instead of over a worklist
_WORKLISTS = os.environ.get("DEEPEMIA_MASK_WORKLISTS", "1") != "0"


def _points_into(cs: "ContourSet", out: torch.Tensor, out_c: int, um_pix: float, sel: Optional[np.ndarray], entry: str, work_ints: str) -> None:
    """One launch of a POINT-TABLE family's entry (``demia_contour_shape``) into ``out`` [M, out_c, cols]: every mask, or the
    positions ``sel`` (a flag per mask over the full tables; the other rows are left as they are)."""
    ops = cs.ops
    M, C, mp = cs.M, cs.C, cs.max_points
    wi = torch.empty((int(getattr(ops.lib, work_ints)(M, C, mp)),), dtype=torch.int32, device=ops.device)
    _lib.check(getattr(ops.lib, entry)(_lib.ptr(cs._flags(sel)), _lib.ptr(cs.count), _lib.ptr(cs.info), _lib.ptr(cs.red), _lib.ptr(cs.points),
                                       M, C, mp, _lib.ptr(wi), float(um_pix), _lib.ptr(out), int(out_c), ops._stream()), entry)


def _words_into(cs: "ContourSet", out: torch.Tensor, out_c: int, um_pix: float, sel: Optional[np.ndarray], what: str, entries: Tuple[str, str],
                second_scratch: bool = False) -> None:
    """One launch of a WORD family's entry (``entries``: for planes, for crops) into ``out`` [M, out_c, cols]: every mask, or the
    positions ``sel`` -- their table rows are gathered, their words are read where they are (the entry's ``select``), their values
    are scattered to their rows of ``out`` and the other rows are left as they are.  ``second_scratch`` (skeleton): the entries
    take one more scratch, made on first use (planes: one more plane per mask, here; crops: ``CropMaskSet.skeleton_scratch``), and
    a thin-only flag, 0."""
    ops = cs.ops
    if cs._words is None:
        raise RuntimeError(f"{what} descriptors: the trace did not keep its words (trace(..., keep_words=True))")
    n = cs.M if sel is None else len(sel)
    if n == 0:
        return
    count, info, sel_d, idx, dst = cs.count, cs.info, None, None, out
    if sel is not None:
        sel_d = ops.upload(np.ascontiguousarray(sel, dtype=np.int32))
        idx = sel_d.to(torch.int64)
        count, info = cs.count.index_select(0, idx), cs.info.index_select(0, idx)
        dst = torch.zeros((n, int(out_c), int(out.shape[2])), dtype=torch.float64, device=ops.device)
    tail = ()
    if cs._words[0] == "plane":
        _, packed, bbox, scratch, W = cs._words
        bb = bbox if idx is None else bbox.index_select(0, idx)
        if second_scratch:
            if cs._scratch2 is None:
                cs._scratch2 = torch.empty_like(packed)          # only touched by regions that do not fit in LDS
            tail = (_lib.ptr(cs._scratch2), 0)
        _lib.check(getattr(ops.lib, entries[0])(_lib.ptr(sel_d), _lib.ptr(packed), _lib.ptr(scratch), _lib.ptr(bb), _lib.ptr(count),
                                                _lib.ptr(info), n, int(packed.shape[1]), W, cs.C, float(um_pix), _lib.ptr(dst), int(out_c),
                                                *tail, ops._stream()), entries[0])
    else:
        _, cset, first = cs._words
        bb = cset.bbox[first:first + cs.M]
        if idx is not None:
            bb, sel_d = bb.index_select(0, idx), sel_d + first
        elif first:
            sel_d = torch.arange(first, first + cs.M, dtype=torch.int32, device=ops.device)
        scratch, off_d = cset.inscribed_scratch()
        if second_scratch:
            scratch2, off2_d = cset.skeleton_scratch()
            tail = (_lib.ptr(scratch2), _lib.ptr(off2_d), 0)
        _lib.check(getattr(ops.lib, entries[1])(_lib.ptr(sel_d), _lib.ptr(cset.payload), _lib.ptr(cset.room), _lib.ptr(cset.offsets),
                                                _lib.ptr(bb), _lib.ptr(count), _lib.ptr(info), n, cset.hw[0], cset.hw[1], cs.C,
                                                float(um_pix), _lib.ptr(dst), int(out_c), _lib.ptr(scratch), _lib.ptr(off_d), *tail,
                                                ops._stream()), entries[1])
    if idx is not None:
        out[idx] = dst


@dataclass(frozen=True)
class Family:
    """One opt-in descriptor family per contour: all that ``ContourSet``, the callers' ``descriptors`` arguments and the CSV
    writer know of it."""
    name: str                # record key, ``inference_settings.<name>_descriptors``
    cols: int                # float64 values per contour
    words: bool              # reads the mask words (the trace must keep them) instead of the point tables
    enqueue: Callable        # (cs, out [M, out_c, cols], out_c, um_pix, sel: positions or None) -> None, without a wait


# in the order of the float64 block of ContourSet.fetch and of the CSV columns
FAMILIES = {f.name: f for f in (
    Family("shape", 10, False, partial(_points_into, entry="demia_contour_shape", work_ints="demia_contour_shape_work_ints")),
    Family("inscribed", 8, True, partial(_words_into, what="inscribed", entries=("demia_mask_inscribed", "demia_crop_inscribed"))),
    Family("skeleton", 8, True, partial(_words_into, what="skeleton", entries=("demia_mask_skeleton", "demia_crop_skeleton"),
                                        second_scratch=True)),
)}


def families(descriptors: Sequence[str]) -> Tuple[Family, ...]:
    """The families named in ``descriptors``, in table order; ``ValueError`` for a name the table does not hold."""
    names = tuple(descriptors)
    unknown = [n for n in names if n not in FAMILIES]
    if unknown:
        raise ValueError(f"unknown descriptor family {unknown[0]!r}: one of {', '.join(FAMILIES)}")
    return tuple(f for f in FAMILIES.values() if f.name in names)


def reads_words(descriptors: Sequence[str]) -> bool:
    """Whether any of the families ``descriptors`` reads the mask words: the trace then has to keep them."""
    return any(f.words for f in families(descriptors))


@dataclass
class Launched:
    """What ``ContourSet.launch`` enqueued for one family."""
    dev: torch.Tensor                        # [M, slots, cols] float64 on the device
    slots: int
    um_pix: float
    host: Optional[np.ndarray] = None        # [M, max contours per mask, cols] view of fetch()'s copy; None when it fell back


def neighbour_offsets(area) -> np.ndarray:
    """``point_off`` [M + 1] i64 of ``demia_mask_neighbours``: the exclusive prefix sum of the masks' pixel counts on the host (a
    mask has no more border pixels than pixels), so the border points need no count-then-allocate wait."""
    a = np.maximum(np.asarray(area, dtype=np.int64).reshape(-1), 0)
    off = np.zeros(len(a) + 1, dtype=np.int64)
    np.cumsum(a, out=off[1:])
    return off


@dataclass
class Neighbours:
    """What ``MaskOps.neighbours`` / ``CropMaskSet.neighbours`` enqueued (``demia_mask_neighbours``), all on the device."""
    table: torch.Tensor          # [M, 6] int64: d2_any, idx_any, d2_group, idx_group, touching, within
    sums: torch.Tensor           # [M, 3] int64: N, Sx, Sy
    nborder: torch.Tensor        # [M] int32
    points: torch.Tensor         # int32 words: mask m's border pixels (y << 16 | x) from point_off[m]
    point_off: np.ndarray        # [M + 1] int64, on the host
    point_off_dev: Optional[torch.Tensor] = None             # ... and where the stage uploaded it (the agglomerate stage reuses it)

    # int32 views of the two tables: what rides in ContourSet.fetch(extra=...)
    @property
    def table_i32(self) -> torch.Tensor:
        return self.table.view(torch.int32)

    @property
    def sums_i32(self) -> torch.Tensor:
        return self.sums.view(torch.int32)

    @property
    def ride(self) -> List[torch.Tensor]:
        return [self.table_i32, self.sums_i32]

    @staticmethod
    def from_i32(table_i32: np.ndarray, sums_i32: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """The host copies of :attr:`table_i32` / :attr:`sums_i32` as the int64 tables ``[M, 6]`` / ``[M, 3]``."""
        t = np.ascontiguousarray(table_i32, dtype=np.int32).reshape(-1).view(np.int64).reshape(-1, 6)
        s = np.ascontiguousarray(sums_i32, dtype=np.int32).reshape(-1).view(np.int64).reshape(-1, 3)
        return t, s


def _neighbour_buffers(ops: "MaskOps", M: int, area, group,
                       with_table: bool = True) -> Tuple[Neighbours, Optional[torch.Tensor], torch.Tensor]:
    """The outputs of one neighbour stage and its two host tables on the device, in ONE upload: (result, group or None, point_off).
    ``with_table`` false: the border stage alone, for a caller that pairs the points itself."""
    off = neighbour_offsets(area)
    assert len(off) == M + 1
    dev = ops.device
    res = Neighbours(torch.empty((M, 6), dtype=torch.int64, device=dev) if with_table else None,
                     torch.empty((M, 3), dtype=torch.int64, device=dev),
                     torch.empty((M,), dtype=torch.int32, device=dev), torch.empty((max(int(off[-1]), 1),), dtype=torch.int32, device=dev), off)
    parts = [off.view(np.int32)]
    if group is not None:
        g = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
        assert len(g) == M
        parts.append(g)
    tab = ops.upload(np.concatenate(parts))
    res.point_off_dev = tab[:2 * (M + 1)].view(torch.int64)
    return res, (tab[2 * (M + 1):] if group is not None else None), res.point_off_dev


def _launch_neighbours(ops: "MaskOps", entry: str, source: Sequence[Optional[torch.Tensor]], M: int, H: int, W: int, area, group,
                       r2: int) -> Neighbours:
    """One neighbour stage, enqueued without a wait.  ``entry`` and ``source``, the entry's leading word-source arguments:
    ``demia_mask_neighbours`` with planes ``(packed, bbox)`` or ``demia_crop_neighbours`` with crops ``(payload, room, offsets,
    bbox)``.  ``area``: the pixel counts on the host."""
    res, group_d, off_d = _neighbour_buffers(ops, M, area, group)
    _lib.check(getattr(ops.lib, entry)(*(_lib.ptr(t) for t in source), _lib.ptr(group_d), M, H, W, int(r2), _lib.ptr(off_d),
                                       _lib.ptr(res.points), _lib.ptr(res.nborder), _lib.ptr(res.sums), _lib.ptr(res.table),
                                       ops._stream()), entry)
    return res


@dataclass
class Agglomerates:
    """What ``MaskOps.agglomerates`` / ``CropMaskSet.agglomerates`` enqueued (``demia_mask_agglomerates``), all on the device."""
    links: torch.Tensor          # [M, ceil(M / 32)] int32 words: bit b of row a = link(a, b); stays on the device
    degree: torch.Tensor         # [M] int32
    label: torch.Tensor          # [M] int32: the smallest index of the mask's component, -1 without a pixel
    own: torch.Tensor            # [M, 6] int64: N, Sx, Sy, Sxx, Syy, Sxy of the pixels no linked lower mask holds
    sums: torch.Tensor           # [M, 3] int64, nborder, points, point_off: the border stage's (a Neighbours' own when reused)
    nborder: torch.Tensor
    points: torch.Tensor
    point_off: np.ndarray

    # int32 views of the three small tables: what rides in ContourSet.fetch(extra=...), 56 bytes per mask
    @property
    def ride(self) -> List[torch.Tensor]:
        return [self.label, self.degree, self.own.view(torch.int32)]

    @staticmethod
    def from_i32(label_i32: np.ndarray, degree_i32: np.ndarray, own_i32: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The host copies of the ride as ``label`` [M] int32, ``degree`` [M] int32 and ``own`` [M, 6] int64."""
        lab = np.ascontiguousarray(label_i32, dtype=np.int32).reshape(-1)
        deg = np.ascontiguousarray(degree_i32, dtype=np.int32).reshape(-1)
        own = np.ascontiguousarray(own_i32, dtype=np.int32).reshape(-1).view(np.int64).reshape(-1, 6)
        return lab, deg, own


def _launch_agglomerates(ops: "MaskOps", entry: str, source: Sequence[Optional[torch.Tensor]], M: int, H: int, W: int, area, group,
                         l2: int, border: Optional[Neighbours], label_lds_cap: int) -> Agglomerates:
    """One agglomerate stage, enqueued without a wait; ``entry`` and ``source`` as for ``_launch_neighbours``
    (``demia_mask_agglomerates`` / ``demia_crop_agglomerates``).  Without ``border`` the border tensors and the one upload are
    those of a neighbour stage (its pair table is not made); with it -- a ``Neighbours`` of the same masks -- its border tensors
    and its uploaded ``point_off`` are reused and only ``group``, if any, is uploaded."""
    dev = ops.device
    wpl = (M + 31) // 32
    if border is not None:
        assert len(border.point_off) == M + 1 and border.point_off_dev is not None
        nb, off_d, group_d = border, border.point_off_dev, None
        if group is not None and M:
            g = np.ascontiguousarray(group, dtype=np.int32).reshape(-1)
            assert len(g) == M
            group_d = ops.upload(g)
    else:
        nb, group_d, off_d = _neighbour_buffers(ops, M, area, group, with_table=False)
    res = Agglomerates(torch.empty((M, wpl), dtype=torch.int32, device=dev), torch.empty((M,), dtype=torch.int32, device=dev),
                       torch.empty((M,), dtype=torch.int32, device=dev), torch.empty((M, 6), dtype=torch.int64, device=dev),
                       nb.sums, nb.nborder, nb.points, nb.point_off)
    _lib.check(getattr(ops.lib, entry)(*(_lib.ptr(t) for t in source), _lib.ptr(group_d), M, H, W, int(l2), _lib.ptr(off_d),
                                       _lib.ptr(res.points), _lib.ptr(res.nborder), _lib.ptr(res.sums), int(border is not None),
                                       _lib.ptr(res.links), _lib.ptr(res.degree), _lib.ptr(res.label), _lib.ptr(res.own),
                                       int(label_lds_cap), ops._stream()), entry)
    return res


OUTLINE_BINS = 128                       # bins of the distance histogram of demia_mask_outline_agreement; the last one saturates
OUTLINE_REC = 8 + OUTLINE_BINS           # int32 words of one record


@dataclass
class OutlineAgreement:
    """What ``MaskOps.outline_agreement`` / ``CropMaskSet.outline_agreement`` enqueued (``demia_mask_outline_agreement``; the
    definitions are in ``include/deepemia_hip.h``), all on the device.  ``records`` is the whole result: a fixed size per pair, so
    one copy brings it over and :meth:`from_host` decodes it."""
    records: torch.Tensor        # [P, 2, OUTLINE_REC] int32: per pair and direction (0: detection -> annotation, 1: the reverse)
    pairs: np.ndarray            # [P, 2] int32 on the host: detection index, annotation index
    det: Optional[Neighbours] = None         # the border stages' outputs (table None); they stay on the device
    gt: Optional[Neighbours] = None

    @staticmethod
    def from_host(records_i32: np.ndarray) -> Dict[str, np.ndarray]:
        """The host copy of :attr:`records` as int64 arrays: ``n``, ``max_d2``, ``sum_d2``, ``sum_q`` ``[P, 2]`` and ``hist``
        ``[P, 2, 128]``."""
        r = np.ascontiguousarray(records_i32, dtype=np.int32).reshape(-1, 2, OUTLINE_REC)
        head = np.ascontiguousarray(r[:, :, :8]).view(np.int64).reshape(-1, 2, 4)
        return {"n": head[:, :, 0].copy(), "max_d2": head[:, :, 1].copy(), "sum_d2": head[:, :, 2].copy(), "sum_q": head[:, :, 3].copy(),
                "hist": r[:, :, 8:].astype(np.int64)}


def _launch_outline(ops: "MaskOps", entry: str, det_source: Sequence[Optional[torch.Tensor]], D: int, det_area,
                    gt_source: Sequence[Optional[torch.Tensor]], G: int, gt_area, H: int, W: int, pairs) -> OutlineAgreement:
    """One outline-agreement stage, enqueued without a wait.  ``entry`` with the leading word-source arguments of both sides:
    ``demia_mask_outline_agreement`` with planes ``(packed, bbox)`` or ``demia_crop_outline_agreement`` with crops ``(payload, room,
    offsets, bbox)``.  ``det_area`` / ``gt_area``: the pixel counts on the host (they size the border points and the grid);
    ``pairs``: ``[P, 2]`` on the host.  The four host tables go up in ONE upload.  Without a pair, or with an empty side, nothing
    is allocated beyond the empty result and nothing is launched."""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    P = int(pairs.shape[0])
    dev = ops.device
    if P == 0 or D == 0 or G == 0:
        return OutlineAgreement(torch.zeros((P, 2, OUTLINE_REC), dtype=torch.int32, device=dev), pairs)
    if pairs[:, 0].min() < 0 or pairs[:, 0].max() >= D or pairs[:, 1].min() < 0 or pairs[:, 1].max() >= G:
        raise ValueError(f"outline_agreement: a pair names a mask outside its set ({D} detections, {G} annotations)")
    d_area = np.ascontiguousarray(np.maximum(np.asarray(det_area, dtype=np.int64).reshape(-1), 0))
    g_area = np.ascontiguousarray(np.maximum(np.asarray(gt_area, dtype=np.int64).reshape(-1), 0))
    assert len(d_area) == D and len(g_area) == G
    d_off, g_off = neighbour_offsets(d_area), neighbour_offsets(g_area)
    chunk_off = np.zeros(2 * P + 1, dtype=np.int64)
    n_chunks = int(ops.lib.demia_outline_chunks(d_area.ctypes.data, D, g_area.ctypes.data, G, pairs.ctypes.data, P, chunk_off.ctypes.data))
    tab = ops.upload(np.concatenate([d_off.view(np.int32), g_off.view(np.int32), chunk_off.view(np.int32), pairs.reshape(-1)]))
    a, b, c = 2 * (D + 1), 2 * (D + 1) + 2 * (G + 1), 2 * (D + 1) + 2 * (G + 1) + 2 * (2 * P + 1)
    d_off_d, g_off_d, chunk_d, pairs_d = tab[:a].view(torch.int64), tab[a:b].view(torch.int64), tab[b:c].view(torch.int64), tab[c:]

    def border(M: int, off: np.ndarray, off_d: torch.Tensor) -> Neighbours:
        return Neighbours(None, torch.empty((M, 3), dtype=torch.int64, device=dev), torch.empty((M,), dtype=torch.int32, device=dev),
                          torch.empty((max(int(off[-1]), 1),), dtype=torch.int32, device=dev), off, off_d)
    det, gt = border(D, d_off, d_off_d), border(G, g_off, g_off_d)
    records = torch.zeros((P, 2, OUTLINE_REC), dtype=torch.int32, device=dev)       # (the entry's contract: the caller zeroes)
    _lib.check(getattr(ops.lib, entry)(*(_lib.ptr(t) for t in det_source), D, *(_lib.ptr(t) for t in gt_source), G, H, W,
                                       _lib.ptr(d_off_d), _lib.ptr(det.points), _lib.ptr(det.nborder), _lib.ptr(det.sums),
                                       _lib.ptr(g_off_d), _lib.ptr(gt.points), _lib.ptr(gt.nborder), _lib.ptr(gt.sums),
                                       _lib.ptr(pairs_d), P, _lib.ptr(chunk_d), n_chunks, _lib.ptr(records), ops._stream()), entry)
    return OutlineAgreement(records, pairs, det, gt)


def _launch_error_map(ops: "MaskOps", entry: str, det_source: Sequence[Optional[torch.Tensor]], D: int, d_state,
                      gt_source: Sequence[Optional[torch.Tensor]], G: int, g_state, H: int, W: int, image: torch.Tensor,
                      alpha, line, palette) -> Tuple[torch.Tensor, torch.Tensor]:
    """One error-map stage, enqueued without a wait: ``(dst [H, W, 3] u8, counts [4] i64)`` on the device.  ``entry`` with the
    leading word-source arguments of both sides, as for :func:`_launch_outline`: ``demia_mask_error_map`` with planes ``(packed,
    bbox)`` or ``demia_crop_error_map`` with crops ``(payload, room, offsets, bbox)``.  ``d_state`` / ``g_state`` are host arrays and
    go up in ONE upload.  Every argument is checked before anything is allocated or launched: ValueError."""
    if isinstance(alpha, bool) or not isinstance(alpha, (int, np.integer)) or not (0 <= int(alpha) <= 256):
        raise ValueError(f"error_map: alpha must be an integer from 0 to 256, got {alpha!r}")
    if isinstance(line, bool) or not isinstance(line, (int, np.integer)) or not (1 <= int(line) <= 4):
        raise ValueError(f"error_map: line must be an integer from 1 to 4, got {line!r}")
    if palette is None:
        from .cocoeval import ERROR_MAP_PALETTE          # (the one table of the defaults)
        palette = ERROR_MAP_PALETTE
    try:
        pal = np.asarray(palette)
        ok = pal.shape == (8, 3) and pal.dtype.kind in "iu" and int(pal.min()) >= 0 and int(pal.max()) <= 255
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("error_map: the palette must be 8 BGR triples of bytes")
    pal = np.ascontiguousarray(pal, dtype=np.uint8)
    if not isinstance(image, torch.Tensor) or image.dtype != torch.uint8 or image.device != ops.device or \
            tuple(image.shape) not in ((H, W), (H, W, 1), (H, W, 3)):
        got = tuple(image.shape) if isinstance(image, torch.Tensor) else type(image).__name__
        raise ValueError(f"error_map: the image must be a uint8 device tensor of the frame, [{H}, {W}] or [{H}, {W}, 1 | 3], got {got}")
    if not (0 < H <= 65535 and 0 < W <= 65535):
        raise ValueError(f"error_map: a frame of {(H, W)}")
    states = []
    for name, st, n, top in (("d_state", d_state, D, 2), ("g_state", g_state, G, 3)):
        st = np.asarray(st).reshape(-1)
        if len(st) != n or (n and (st.dtype.kind not in "iu" or int(st.min()) < 0 or int(st.max()) > top)):
            raise ValueError(f"error_map: {name} must be {n} integers from 0 to {top}")
        states.append(st.astype(np.int32))
    image = image.contiguous()
    C = 3 if image.dim() == 3 and int(image.shape[2]) == 3 else 1
    dev = ops.device
    st_d = ops.upload(np.concatenate(states)) if D + G else torch.zeros((0,), dtype=torch.int32, device=dev)
    dst = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    counts = torch.empty((4,), dtype=torch.int64, device=dev)
    partial = torch.empty((int(ops.lib.demia_error_map_tiles(H, W)), 4), dtype=torch.int64, device=dev)
    _lib.check(getattr(ops.lib, entry)(*(_lib.ptr(t) for t in det_source), _lib.ptr(st_d[:D]) if D else 0, D,
                                       *(_lib.ptr(t) for t in gt_source), _lib.ptr(st_d[D:]) if G else 0, G, H, W, _lib.ptr(image), C,
                                       _lib.ptr(dst), int(alpha), int(line), pal.ctypes.data, _lib.ptr(partial), _lib.ptr(counts),
                                       ops._stream()), entry)
    return dst, counts


class PlanePool:
    """Mask planes that stay ZERO outside per-slot boxes (``demia_mask_gather_regions_pooled``): a gather into the pool
    writes the union of a slot's previous box and its new one instead of whole 512-KiB planes.  The planes handed out are
    views of the pool -- valid until the pool is used again (callers that keep masks longer take fresh planes)."""

    def __init__(self, device, H: int, wpr: int, cap: int):
        self.H, self.wpr, self.cap = int(H), int(wpr), int(cap)
        self.planes = torch.zeros((self.cap, self.H, self.wpr), dtype=torch.int32, device=device)
        self.prev = torch.full((self.cap, 4), -1, dtype=torch.int32, device=device)

    def fits(self, n: int, H: int, wpr: int) -> bool:
        return n <= self.cap and (H, wpr) == (self.H, self.wpr)


class MaskOps:
    """Thin, stateless wrapper of the packed-mask entry points for one device."""

    def __init__(self, device: str = "cuda:0"):
        if not torch.cuda.is_available():
            raise _lib.HipExtensionMissing("no HIP device visible: packed-mask ops have no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device(device)
        self._frame_w = 0
        self._points_hint = 0             # contour points the previous trace used (+ slack): sizes ContourSet.fetch(with_points=True)
        self._protected = []              # (first byte, last byte) of planes the in-place ops must never touch (see protect)

    def protect(self, planes: torch.Tensor) -> None:
        """Register planes that consumers may only READ: a captured forward's own output planes stay zero outside the boxes its
        next replay knows about (incremental paste), so an in-place stage on them would leave bits no replay ever clears."""
        import weakref
        lo = int(planes.data_ptr())
        rng = (lo, lo + planes.numel() * planes.element_size())
        if not any(r[:2] == rng and r[2]() is not None for r in self._protected):
            # the registration lives as long as the planes' own tensor (the graph's static buffer, `_base` of the view handed out):
            # when the engine evicts the shape and the memory is reused, the range is no longer protected
            owner = planes._base if planes._base is not None else planes
            self._protected.append(rng + (weakref.ref(owner),))

    def unprotect(self, planes: torch.Tensor) -> None:
        lo = int(planes.data_ptr())
        self._protected = [r for r in self._protected if r[0] != lo]

    def _writable(self, packed: torch.Tensor, what: str) -> None:
        """Every in-place op (``program_``, ``overlap_prefix_``) calls this first."""
        if not self._protected:
            return
        self._protected = [r for r in self._protected if r[2]() is not None]
        p = int(packed.data_ptr())
        for lo, hi, _ in self._protected:
            if lo <= p < hi:
                raise RuntimeError(f"{what}: in-place stage on the read-only output planes of a captured forward -- gather a copy first")

    def set_frame_width(self, W: int) -> None:
        """True pixel width of the full-frame masks in flight.  Packed rows hold ceil(W / 32) words; kernels need
        the true W for the right border (replicate rule of the morphology, image-frame seeds of the hole fill).
        Tensors whose row length does not match ceil(W / 32) (tile-level masks) are taken as 32 * words wide."""
        self._frame_w = int(W)

    def _w(self, packed: torch.Tensor) -> int:
        wpr = int(packed.shape[-1])
        return self._frame_w if (self._frame_w and (self._frame_w + 31) // 32 == wpr) else wpr * 32

    def _stream(self) -> int:
        return int(torch.cuda.current_stream(self.device).cuda_stream)

    def upload(self, arr: np.ndarray) -> torch.Tensor:
        """Host table -> device WITHOUT queueing the host behind the current stream's backlog: a copy from pageable memory
        returns only when it has run, and on the post-processing stream that means after every kernel already enqueued
        there (each of which waits for a CU beside the resident convolution workgroups).  The copy goes through a side
        stream that is always empty; the current stream waits for its event."""
        t = torch.from_numpy(np.ascontiguousarray(arr))
        cur = torch.cuda.current_stream(self.device)
        if getattr(self, "_up_stream", None) is None:
            self._up_stream = torch.cuda.Stream(device=self.device)
        # (set_stream, not `with torch.cuda.stream(...)`: that context asks torch.cuda.is_available() -- hipGetDeviceCount, ~0.1 ms --
        # three times per use, and this runs two dozen times per image: 5 ms of a 36-ms image in the round-5 profile)
        torch.cuda.set_stream(self._up_stream)
        try:
            d = t.to(self.device)
            ev = torch.cuda.Event()
            ev.record(self._up_stream)
        finally:
            torch.cuda.set_stream(cur)
        cur.wait_event(ev)
        d.record_stream(cur)
        return d

    # -- construction -------------------------------------------------------------------------
    def from_dense(self, masks: np.ndarray) -> torch.Tensor:
        """(M, H, W) bool/uint8 host array -> packed device tensor (test / interop helper)."""
        m = np.ascontiguousarray(masks != 0)
        M, H, W = m.shape
        wpr = (W + 31) // 32
        if W % 32:
            m = np.concatenate([m, np.zeros((M, H, wpr * 32 - W), dtype=bool)], axis=2)
        packed = np.packbits(m.reshape(M, H, wpr, 32), axis=-1, bitorder="little").view(np.uint32)
        return torch.from_numpy(packed.reshape(M, H, wpr).view(np.int32)).to(self.device)

    def to_dense(self, packed: torch.Tensor, W: int) -> np.ndarray:
        M, H, wpr = packed.shape
        out = torch.empty((M, H, W), dtype=torch.bool, device=self.device)
        _lib.check(self.lib.demia_unpack_masks(_lib.ptr(packed), _lib.ptr(out), M, H, W, self._stream()), "demia_unpack_masks")
        return out.cpu().numpy()

    # -- reductions -----------------------------------------------------------------------------
    def area_bbox(self, packed: torch.Tensor, hint: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Pixel count and tight bbox per mask.  ``hint`` ([M, 4] int32 boxes known to contain the masks, e.g. the
        paste boxes) restricts the scan to those regions instead of the whole frame."""
        M, H, wpr = packed.shape
        area = torch.empty((M,), dtype=torch.int32, device=self.device)
        bbox = torch.empty((M, 4), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.demia_mask_area_bbox(_lib.ptr(packed), _lib.ptr(hint), _lib.ptr(area), _lib.ptr(bbox), M, H,
                                                 self._w(packed), self._stream()), "demia_mask_area_bbox")
        return area, bbox

    def column_counts(self, packed: torch.Tensor, seg: Optional[torch.Tensor] = None, n_seg: int = 1,
                      bbox: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Per-column pixel counts over all masks ([W]), or per segment ([n_seg, W]) when ``seg`` (int32,
        non-decreasing segment id per mask) is given.  At most 65535 masks per call (one grid row per mask): the C side
        refuses more with an error, it does not split the call."""
        M, H, wpr = packed.shape
        W = self._w(packed)
        shape = (W,) if seg is None else (n_seg, W)
        counts = torch.zeros(shape, dtype=torch.int32, device=self.device)
        if bbox is None:
            _, bbox = self.area_bbox(packed)
        _lib.check(self.lib.demia_mask_column_counts(_lib.ptr(packed), _lib.ptr(seg), _lib.ptr(bbox), M, H, W,
                                                     _lib.ptr(counts), self._stream()), "demia_mask_column_counts")
        return counts

    def pair_intersections(self, a: torch.Tensor, b: torch.Tensor, bbox_a: torch.Tensor, bbox_b: torch.Tensor,
                           pi: np.ndarray, pj: np.ndarray) -> np.ndarray:
        P = len(pi)
        if P == 0:
            return np.zeros((0,), dtype=np.int64)
        _, H, wpr = a.shape
        ti = torch.from_numpy(np.ascontiguousarray(pi, dtype=np.int32)).to(self.device)
        tj = torch.from_numpy(np.ascontiguousarray(pj, dtype=np.int32)).to(self.device)
        out = torch.empty((P,), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.demia_mask_pair_intersections(_lib.ptr(a), _lib.ptr(b), _lib.ptr(ti), _lib.ptr(tj), _lib.ptr(bbox_a),
                                                          _lib.ptr(bbox_b), _lib.ptr(out), P, H, self._w(a), self._stream()),
                   "demia_mask_pair_intersections")
        return out.cpu().numpy().astype(np.int64)

    def pair_matrix(self, packed: torch.Tensor, bbox: torch.Tensor, first: np.ndarray, count: np.ndarray,
                    label: Optional[np.ndarray] = None, ld: Optional[int] = None) -> torch.Tensor:
        """[M, ld] int32 ON THE DEVICE: row i, column j - first[i] = |mask_i & mask_j| for every j > i of mask i's segment
        (``first[i]`` / ``count[i]``: start and length of that segment; ``label``: equal-label pairs only).  The pair
        list is made on the device from the boxes -- no host round trip between the stage that reduces the boxes and the
        counts (``demia_mask_pair_matrix``).  The caller fetches it together with whatever else it waits for."""
        M, H, wpr = packed.shape
        if ld is None:
            ld = max(1, int(np.max(count)) if M else 1)
        out = torch.zeros((M, ld), dtype=torch.int32, device=self.device)
        if M == 0:
            return out
        tab = np.stack([np.asarray(first, dtype=np.int32), np.asarray(count, dtype=np.int32),
                        np.asarray(label if label is not None else np.zeros(M), dtype=np.int32)])
        tt = self.upload(tab)
        _lib.check(self.lib.demia_mask_pair_matrix(_lib.ptr(packed), _lib.ptr(bbox), _lib.ptr(tt[0]), _lib.ptr(tt[1]),
                                                   _lib.ptr(tt[2]) if label is not None else 0, _lib.ptr(out), M, ld, H, self._w(packed),
                                                   self._stream()), "demia_mask_pair_matrix")
        return out

    def gray_histogram(self, packed: torch.Tensor, image: torch.Tensor, bbox: Optional[torch.Tensor] = None) -> np.ndarray:
        """[M, 256] gray-level counts of ``image`` ([H, W, 3] BGR or [H, W] gray, uint8, on the device) under each mask:
        what ``np.histogram(cv2.cvtColor(image, BGR2GRAY)[mask > 0], bins=256, range=(0, 255))`` counts
        (measurements.py:197-205)."""
        M, H, wpr = packed.shape
        if M == 0:
            return np.zeros((0, 256), dtype=np.int64)
        W = self._w(packed)
        assert image.dtype == torch.uint8 and image.is_contiguous() and tuple(image.shape[:2]) == (H, W), (image.shape, H, W)
        ch = 1 if image.dim() == 2 else int(image.shape[2])
        if bbox is None:
            _, bbox = self.area_bbox(packed)
        hist = torch.empty((M, 256), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.demia_mask_gray_histogram(_lib.ptr(packed), _lib.ptr(bbox), _lib.ptr(image), ch, M, H, W,
                                                      _lib.ptr(hist), self._stream()), "demia_mask_gray_histogram")
        return hist.cpu().numpy().astype(np.int64)

    # -- morphology -----------------------------------------------------------------------------
    def program_(self, packed: torch.Tensor, stages: Sequence[str], bbox: Optional[torch.Tensor] = None,
                 active: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Run per-mask stages IN PLACE on the bbox region of every mask (``demia_mask_program``): ``stages`` from
        ``fill``, ``dilate``, ``erode``, ``drop_multi``, ``flag_multi``, ``gate`` (masks with ``active[m] == 0`` stop
        there).  ``bbox`` may be any superset of the tight boxes.  Returns (area, tight bbox, multi-component flag) of
        the result."""
        M, H, wpr = packed.shape
        assert len(stages) <= 8 and packed.is_contiguous()
        prog = 0
        for i, st in enumerate(stages):
            prog |= _lib.MOP[st] << (4 * i)
        if bbox is None:
            _, bbox = self.area_bbox(packed)
        area = torch.empty((M,), dtype=torch.int32, device=self.device)
        bbox_out = torch.empty((M, 4), dtype=torch.int32, device=self.device)
        flag = torch.empty((M,), dtype=torch.int32, device=self.device)
        scratch = torch.empty_like(packed)       # only touched by regions that do not fit in LDS
        worklist = torch.empty((M + 2,), dtype=torch.int32, device=self.device) if _WORKLISTS else None    # masks for the large-region variant
        _lib.check(self.lib.demia_mask_program_wl(_lib.ptr(packed), _lib.ptr(scratch), _lib.ptr(bbox), _lib.ptr(active), prog, M, H,
                                                  self._w(packed), _lib.ptr(area), _lib.ptr(bbox_out), _lib.ptr(flag),
                                                  _lib.ptr(worklist), self._stream()), "demia_mask_program_wl")
        return area, bbox_out, flag

    def fill_holes(self, packed: torch.Tensor, bbox: Optional[torch.Tensor] = None) -> torch.Tensor:
        out = packed.clone()
        self.program_(out, ["fill"], bbox)
        return out

    def erode(self, packed: torch.Tensor, bbox: Optional[torch.Tensor] = None) -> torch.Tensor:
        out = packed.clone()
        self.program_(out, ["erode"], bbox)
        return out

    def dilate(self, packed: torch.Tensor, bbox: Optional[torch.Tensor] = None) -> torch.Tensor:
        out = packed.clone()
        self.program_(out, ["dilate"], bbox)
        return out

    def overlap_prefix_(self, packed: torch.Tensor, seg: Optional[torch.Tensor] = None,
                        bbox: Optional[torch.Tensor] = None) -> torch.Tensor:
        M, H, wpr = packed.shape
        self._writable(packed, "overlap_prefix_")
        _lib.check(self.lib.demia_mask_overlap_prefix(_lib.ptr(packed), _lib.ptr(seg), _lib.ptr(bbox), M, H, self._w(packed),
                                                      self._stream()), "demia_mask_overlap_prefix")
        return packed

    def components_gt1(self, packed: torch.Tensor, bbox: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``label(mask).max() > 1`` per mask (the masks are not changed)."""
        return self.program_(packed, ["flag_multi"], bbox)[2]

    def pool(self, name: str, n: int, H: int, wpr: int) -> PlanePool:
        """The named plane pool, (re)allocated when it is too small or of another frame size."""
        pools = self.__dict__.setdefault("_pools", {})
        p = pools.get(name)
        if p is None or not p.fits(n, H, wpr):
            pools.pop(name, None)
            p = pools[name] = PlanePool(self.device, H, wpr, max(int(n * 1.25) + 64, 256))
        return p

    def gather_regions_pooled(self, src: torch.Tensor, index, bbox, pool: PlanePool, first: int = 0, grow: int = 2) -> torch.Tensor:
        """``src[index]`` into slots ``first ..`` of ``pool`` (see :class:`PlanePool`); returns the view of those slots."""
        idx = index if torch.is_tensor(index) else self.upload(np.asarray(index, dtype=np.int64))
        idx = idx.to(device=self.device, dtype=torch.int64).contiguous()
        bb = bbox if torch.is_tensor(bbox) else self.upload(np.ascontiguousarray(bbox, dtype=np.int32))
        bb = bb.to(device=self.device, dtype=torch.int32).contiguous()
        n = int(idx.shape[0])
        _, H, wpr = src.shape
        assert bb.shape == (n, 4) and src.is_contiguous() and src.dtype == torch.int32 and pool.fits(first + n, H, wpr)
        out = pool.planes[first:first + n]
        _lib.check(self.lib.demia_mask_gather_regions_pooled(_lib.ptr(src), _lib.ptr(idx), _lib.ptr(bb), n, H, self._w(src), _lib.ptr(out),
                                                             _lib.ptr(pool.prev[first:first + n]), int(grow), self._stream()),
                   "demia_mask_gather_regions_pooled")
        return out

    def gather_regions(self, src: torch.Tensor, index, bbox, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``src[index]`` for masks that are zero outside ``bbox`` (a superset of their tight boxes; -1 = empty): reads the
        boxes only, writes each destination plane once.  ``index``: int sequence / array (or an i64 device tensor), ``bbox``
        [n, 4] numpy or i32 device tensor, row i belonging to ``index[i]``."""
        idx = index if torch.is_tensor(index) else self.upload(np.asarray(index, dtype=np.int64))
        idx = idx.to(device=self.device, dtype=torch.int64).contiguous()
        bb = bbox if torch.is_tensor(bbox) else self.upload(np.ascontiguousarray(bbox, dtype=np.int32))
        bb = bb.to(device=self.device, dtype=torch.int32).contiguous()
        n = int(idx.shape[0])
        assert bb.shape == (n, 4) and src.is_contiguous() and src.dtype == torch.int32
        _, H, wpr = src.shape
        if out is None:
            out = torch.empty((n, H, wpr), dtype=torch.int32, device=self.device)
        assert out.is_contiguous() and tuple(out.shape) == (n, H, wpr)
        _lib.check(self.lib.demia_mask_gather_regions(_lib.ptr(src), _lib.ptr(idx), _lib.ptr(bb), n, H, self._w(src), _lib.ptr(out),
                                                      self._stream()), "demia_mask_gather_regions")
        return out

    def place_tiles(self, src: torch.Tensor, x_off: Sequence[int], y_off: Sequence[int], tile_h: int, tile_w: int,
                    H: int, W: int, src_w: Optional[int] = None) -> torch.Tensor:
        """``cv2.resize(mask, (tile_w, tile_h), INTER_NEAREST)`` + paste at (x_off, y_off) into a zero (H, W) frame.
        ``src_w``: true pixel width of the source masks (default: 32 x their words per row)."""
        T, sh, swpr = src.shape
        dst = torch.empty((T, H, (W + 31) // 32), dtype=torch.int32, device=self.device)
        xo = torch.tensor(list(x_off), dtype=torch.int32, device=self.device)
        yo = torch.tensor(list(y_off), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.demia_mask_place_tiles(_lib.ptr(src), _lib.ptr(dst), _lib.ptr(xo), _lib.ptr(yo), T, sh,
                                                   swpr * 32 if src_w is None else int(src_w), tile_h, tile_w, H, W, self._stream()), "demia_mask_place_tiles")
        return dst

    # -- contours + measurements ----------------------------------------------------------------
    def trace(self, packed: torch.Tensor, max_contours: int = 64, max_points: Optional[int] = None,
              bbox: Optional[torch.Tensor] = None, total_area: Optional[int] = None, scratch: Optional[torch.Tensor] = None,
              keep_words: bool = False) -> "ContourSet":
        """cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) + contourArea + arcLength for every mask, once;
        the returned set can be measured later for any subset of its masks without tracing again.  ``bbox`` (any
        superset of the tight boxes) and ``total_area`` (sizes the point pool) save a reduction when known.  ``scratch``:
        the caller's own planes of ``packed``'s shape for the regions that do not fit in LDS (default: allocated here).
        ``keep_words``: the set remembers the planes, the boxes and the scratch it was traced from (the word families of
        ``FAMILIES`` read the words again); the caller leaves them unchanged for as long as it asks the set for their values."""
        M, H, wpr = packed.shape
        W = self._w(packed)
        if bbox is None or (max_points is None and total_area is None):
            area, bbox = self.area_bbox(packed, bbox)
            total_area = int(area.sum().item())
        if max_points is None:
            max_points = int(min(max(4 * int(total_area) // 8 + 4096 * M, 1 << 16), 1 << 26))
        C = max_contours
        cs = ContourSet(self, M, C, max_points)
        if scratch is None:
            scratch = torch.empty_like(packed)   # only touched by regions that do not fit in LDS
        assert scratch.shape == packed.shape and scratch.is_contiguous()
        worklist = torch.empty((M + 2,), dtype=torch.int32, device=self.device) if _WORKLISTS else None    # masks for the large-region variant
        _lib.check(self.lib.demia_mask_contours_wl(_lib.ptr(packed), _lib.ptr(scratch), _lib.ptr(bbox), M, H, W, C, max_points,
                                                   _lib.ptr(cs.count), _lib.ptr(cs.info), _lib.ptr(cs.red), _lib.ptr(cs.points),
                                                   _lib.ptr(cs.counters), _lib.ptr(worklist), self._stream()), "demia_mask_contours_wl")
        if keep_words:
            cs.set_plane_words(packed, bbox, scratch)
        return cs

    def contours(self, packed: torch.Tensor, max_contours: int = 64, max_points: Optional[int] = None,
                 um_pix: float = 1.0, measure: bool = True, bbox: Optional[torch.Tensor] = None, total_area: Optional[int] = None,
                 extra: Optional[Sequence[torch.Tensor]] = None, descriptors: Sequence[str] = ()):
        """Per mask: external contours in OpenCV's order, with area, perimeter and the 12 measurement
        values.  Returns a list (per mask) of lists of dicts with keys ``points`` (P, 2) int32,
        ``area``, ``perimeter`` and (if ``measure``) ``values`` (12,) float64.  ``extra``: int32 device tensors that come to the
        host in the SAME copy (e.g. the cropped words the RLE texts are made of); the call then returns (records, host arrays).
        ``descriptors``: names of ``FAMILIES``; every record also holds each named family's values under its name, (cols,)
        float64, brought over in that same copy."""
        keep_words = reads_words(descriptors)
        if int(packed.shape[0]) == 0:
            return [] if extra is None else ([], [e.cpu().numpy() for e in extra])
        cs = self.trace(packed, max_contours, max_points, bbox=bbox, total_area=total_area, keep_words=keep_words)
        # ONE device-to-host wait: the measurements of every mask's first contours are enqueued right behind the trace and come
        # over with the counts, the contour tables and the points (a mask with more than four contours falls back to the
        # sliced copies of ContourSet.host(): five waits, rare)
        cs.launch_all(um_pix, measure, descriptors, slots=4)
        got = cs.fetch(extra=extra, with_points=True)
        recs = cs.records(um_pix=um_pix, measure=measure, descriptors=descriptors)
        return recs if extra is None else (recs, list(got))

    def neighbours(self, packed: torch.Tensor, bbox: Optional[torch.Tensor], area, group=None, r2: int = -1) -> Neighbours:
        """Nearest edge-to-edge gaps and contact counts between the masks of ``packed`` (``demia_mask_neighbours``; the definition
        is in ``include/deepemia_hip.h``): both kernels are enqueued without a wait and the device tensors returned.  ``bbox``: any
        superset of the tight boxes; ``area``: the pixel counts on the HOST (they size the border points); ``group``: a host array
        of a label per mask, the nearest neighbour is also reported among the masks of the same label (None: one group);
        ``r2``: squared radius of the within count, < 0: not asked for.  With ``area`` (or ``bbox``) None, ``area_bbox`` is read
        with a wait of its own -- for callers outside the pipeline."""
        M, H, wpr = packed.shape
        if M and (area is None or bbox is None):
            a, bbox = self.area_bbox(packed, bbox)
            area = a.cpu().numpy()
        return _launch_neighbours(self, "demia_mask_neighbours", (packed, bbox), M, H, self._w(packed), area if M else np.zeros(0), group, r2)

    def agglomerates(self, packed: torch.Tensor, bbox: Optional[torch.Tensor], area, group=None, l2: int = 2,
                     border: Optional[Neighbours] = None, label_lds_cap: int = 0) -> Agglomerates:
        """The link graph between the masks of ``packed``, its components and the moments that count shared pixels once
        (``demia_mask_agglomerates``; the definitions are in ``include/deepemia_hip.h``): enqueued without a wait, the device
        tensors returned.  ``bbox``, ``area``, ``group``: as for :meth:`neighbours`; ``l2``: the link threshold in squared pixels,
        at least 2; ``border``: the ``Neighbours`` that :meth:`neighbours` returned for the same ``packed``, ``bbox`` and ``area``
        on this stream -- its border points are reused and the border kernel is not launched again."""
        M, H, wpr = packed.shape
        if M and border is None and (area is None or bbox is None):
            a, bbox = self.area_bbox(packed, bbox)
            area = a.cpu().numpy()
        elif M and bbox is None:
            _, bbox = self.area_bbox(packed, bbox)
        return _launch_agglomerates(self, "demia_mask_agglomerates", (packed, bbox), M, H, self._w(packed), area if M else np.zeros(0), group,
                                    l2, border, label_lds_cap)

    def skeleton(self, packed: torch.Tensor, bbox: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The morphological skeleton (Guo-Hall thinning; ``demia_mask_skeleton`` in its thin-only form) of every mask, as packed
        planes of ``packed``'s shape; ``packed`` is left as it is.  ``bbox``: any superset of the tight boxes, when known."""
        M, H, wpr = packed.shape
        out = torch.zeros_like(packed)
        if M == 0:
            return out
        if bbox is None:
            _, bbox = self.area_bbox(packed)
        scratch, scratch2 = torch.empty_like(packed), torch.empty_like(packed)      # only touched by regions that do not fit in LDS
        _lib.check(self.lib.demia_mask_skeleton(0, _lib.ptr(packed), _lib.ptr(scratch), _lib.ptr(bbox), 0, 0, M, H, self._w(packed), 1, 1.0,
                                                0, 0, _lib.ptr(scratch2), _lib.ptr(out), self._stream()), "demia_mask_skeleton")
        return out

    def boundary_band(self, packed: torch.Tensor, bbox: Optional[torch.Tensor], d: int, W: Optional[int] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
        """The boundary band ``m & ~eroded(m, d)`` of every mask (``demia_mask_boundary_band``; the definition is in
        ``include/deepemia_hip.h``): ``(band planes of packed's shape, band_area [M] int32)`` on the device, enqueued without a
        wait; ``packed`` is left as it is.  ``bbox``: any superset of the tight boxes (None: ``area_bbox`` is launched first);
        ``W``: the frame's pixel width (default: ``set_frame_width``'s rule)."""
        M, H, wpr = packed.shape
        d = int(d)
        if d < 1:
            raise ValueError(f"boundary_band: d must be an integer >= 1, got {d}")
        out = torch.zeros_like(packed)
        area = torch.zeros((M,), dtype=torch.int32, device=self.device)
        if M == 0:
            return out, area
        if bbox is None:
            _, bbox = self.area_bbox(packed)
        scratch = torch.empty_like(packed)           # only touched by regions that do not fit in LDS
        if W is not None and (int(W) + 31) // 32 != wpr:
            raise ValueError(f"boundary_band: planes of {wpr} words per row are not {W} pixels wide")
        _lib.check(self.lib.demia_mask_boundary_band(_lib.ptr(packed), _lib.ptr(bbox), M, H, self._w(packed) if W is None else int(W), d, _lib.ptr(out),
                                                     _lib.ptr(area), _lib.ptr(scratch), self._stream()), "demia_mask_boundary_band")
        return out, area

    def outline_agreement(self, det_packed: torch.Tensor, det_bbox: torch.Tensor, det_area, gt_packed: torch.Tensor,
                          gt_bbox: torch.Tensor, gt_area, pairs, W: Optional[int] = None) -> OutlineAgreement:
        """Surface distances between the outlines of the pairs ``pairs`` ``[P, 2]`` (host; detection index, annotation index) of
        two plane sets over one frame, in both directions (``demia_mask_outline_agreement``; the definitions are in
        ``include/deepemia_hip.h``): enqueued without a wait, the device tensors returned.  ``det_bbox`` / ``gt_bbox``: any superset
        of the tight boxes, on the device; ``det_area`` / ``gt_area``: the pixel counts on the HOST; ``W``: the frame's pixel
        width (default: ``set_frame_width``'s rule)."""
        D, H, wpr = det_packed.shape
        G = int(gt_packed.shape[0])
        if G and tuple(gt_packed.shape[1:]) != (H, wpr):
            raise ValueError(f"outline_agreement: planes of {tuple(gt_packed.shape[1:])} against planes of {(H, wpr)}")
        if W is not None and (int(W) + 31) // 32 != wpr:
            raise ValueError(f"outline_agreement: planes of {wpr} words per row are not {W} pixels wide")
        return _launch_outline(self, "demia_mask_outline_agreement", (det_packed, det_bbox), D, det_area, (gt_packed, gt_bbox), G, gt_area,
                               H, self._w(det_packed) if W is None else int(W), pairs)

    def error_map(self, det_packed: torch.Tensor, det_bbox: torch.Tensor, d_state, gt_packed: torch.Tensor, gt_bbox: torch.Tensor,
                  g_state, image: torch.Tensor, alpha: int, line: int, palette=None, W: Optional[int] = None
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
        """The error map of two plane sets over one frame on ``image`` (``demia_mask_error_map``; the definitions are in
        ``include/deepemia_hip.h``): ``(dst [H, W, 3] uint8 BGR, counts [4] int64 = agree, excess, missing, ignored pixels)`` on the
        device, enqueued without a wait; ``image`` (uint8 ``[H, W]``, ``[H, W, 1]`` or ``[H, W, 3]`` BGR, on the device) and the planes
        are left as they are.  ``det_bbox`` / ``gt_bbox``: any superset of the tight boxes, on the device; ``d_state`` (0 not drawn,
        1 matched, 2 unmatched) / ``g_state`` (0 skip, 1 matched, 2 missed, 3 crowd): host arrays; ``alpha`` 0 .. 256; ``line`` 1 .. 4;
        ``palette``: 8 BGR triples (default ``cocoeval.ERROR_MAP_PALETTE``); ``W``: the frame's pixel width (default:
        ``set_frame_width``'s rule).  ValueError for a bad argument, before any launch."""
        D, H, wpr = (int(v) for v in det_packed.shape)
        G = int(gt_packed.shape[0])
        if tuple(gt_packed.shape[1:]) != (H, wpr):
            raise ValueError(f"error_map: planes of {tuple(gt_packed.shape[1:])} against planes of {(H, wpr)}")
        if W is not None and (int(W) + 31) // 32 != wpr:
            raise ValueError(f"error_map: planes of {wpr} words per row are not {W} pixels wide")
        return _launch_error_map(self, "demia_mask_error_map", (det_packed, det_bbox), D, d_state, (gt_packed, gt_bbox), G, g_state,
                                 H, self._w(det_packed) if W is None else int(W), image, alpha, line, palette)


class ContourSet:
    """Device-resident result of one contour trace over M masks (see :meth:`MaskOps.trace`)."""

    def __init__(self, ops: MaskOps, M: int, C: int, max_points: int):
        dev = ops.device
        self.ops, self.M, self.C, self.max_points = ops, M, C, max_points
        self.count = torch.zeros((M,), dtype=torch.int32, device=dev)
        self.info = torch.zeros((M, C, 4), dtype=torch.int32, device=dev)
        self.red = torch.zeros((M, C, 2), dtype=torch.float64, device=dev)
        self.points = torch.empty((max_points, 2), dtype=torch.int32, device=dev)
        self.counters = torch.zeros((4,), dtype=torch.int32, device=dev)
        self._host = None
        self._pts_host = None             # contour points brought over by fetch(with_points=True)
        self._mslots, self._m_um = 4, None    # launch_measure: contour slots per mask and scale of ...
        self._vals_dev = None             # ... the [M, slots, 12] measurement values it enqueued
        self._vals_host = None
        self.launched = {}                # family name -> Launched: what launch() enqueued
        self._words = None                # where the traced words live (set_plane_words / set_crop_words): what the word families read
        self._scratch2 = None             # planes: the second scratch of a word family that wants one, made by its first launch
        self.blocking_point_copies = 0    # times records() had to fetch the points with a device-to-host copy of its own

    def host(self):
        if self._host is None:
            cnt = self.counters.cpu().numpy()
            if cnt[1] != 0:
                raise _lib.HipKernelError(f"contour extraction overflow (flags {int(cnt[1])}): raise max_contours / max_points")
            self.walker_stats = (int(cnt[3]), int(cnt[2]))      # masks traced by parallel walkers, of which fell back
            count = self.count.cpu().numpy()
            # only the contour slots in use cross PCIe ([M, C, ...] with C = 256 is mostly empty: usually one per mask)
            self.max_count = mc = max(1, int(count.max()) if self.M else 1)
            self._host = (count, self.info[:, :mc].contiguous().cpu().numpy(), self.red[:, :mc].contiguous().cpu().numpy(),
                          int(cnt[0]))
        return self._host

    def launch_measure(self, um_pix: float = 1.0, slots: int = 4) -> None:
        """Enqueue the measurements of the first ``slots`` contours of EVERY mask right behind the trace, without waiting
        for the contour counts: :meth:`fetch` then brings counts, contour tables and values to the host with ONE wait.
        (Masks with more contours than ``slots`` -- rare -- are measured again by :meth:`measure` on demand.)"""
        ops = self.ops
        M, C, mp = self.M, self.C, self.max_points
        self._mslots, self._m_um = int(slots), float(um_pix)
        self._wi = torch.empty((int(ops.lib.demia_contour_work_ints(M, C, mp)),), dtype=torch.int32, device=ops.device)
        self._wf = torch.empty((int(ops.lib.demia_contour_work_floats(M, C, mp)),), dtype=torch.float32, device=ops.device)
        self._wd = torch.empty((int(ops.lib.demia_contour_work_doubles(M, C, mp)),), dtype=torch.float64, device=ops.device)
        self._vals_dev = torch.zeros((M, self._mslots, 12), dtype=torch.float64, device=ops.device)
        _lib.check(ops.lib.demia_contour_measure(0, _lib.ptr(self.count), _lib.ptr(self.info), _lib.ptr(self.red),
                                                 _lib.ptr(self.points), M, C, mp, _lib.ptr(self._wi), _lib.ptr(self._wf), _lib.ptr(self._wd),
                                                 float(um_pix), _lib.ptr(self._vals_dev), self._mslots, ops._stream()), "demia_contour_measure")

    def launch(self, name: str, um_pix: float = 1.0, slots: int = 4) -> None:
        """:meth:`launch_measure` for the descriptor family ``name`` of ``FAMILIES``: the first ``slots`` contours of EVERY mask,
        enqueued behind the trace without a wait; :meth:`fetch` carries the values in its one copy, in table order.  (Masks with more
        contours than ``slots`` are computed again by :meth:`descriptor` on demand.)"""
        fam, = families((name,))
        k = min(int(slots), self.C)
        dev = torch.zeros((self.M, k, fam.cols), dtype=torch.float64, device=self.ops.device)
        fam.enqueue(self, dev, k, um_pix, None)
        self.launched[name] = Launched(dev, k, float(um_pix))

    def launch_all(self, um_pix: float, measure: bool, descriptors: Sequence[str], slots: int = 4) -> None:
        """:meth:`launch_measure` if ``measure``, then :meth:`launch` for every family named in ``descriptors``, in table order."""
        fams = families(descriptors)
        if measure:
            self.launch_measure(um_pix, slots=slots)
        for fam in fams:
            self.launch(fam.name, um_pix, slots=slots)

    def set_plane_words(self, packed: torch.Tensor, bbox: torch.Tensor, scratch: torch.Tensor) -> None:
        """This set was traced from the planes ``packed`` with the boxes ``bbox`` and the scratch planes ``scratch``."""
        self._words = ("plane", packed, bbox, scratch, self.ops._w(packed))

    def set_crop_words(self, cset, first: int = 0) -> None:
        """This set is the trace of the masks ``[first, first + M)`` of the crop-framed set ``cset`` -- whether it was traced on the
        words in place or on planes the masks were unpacked into: the payload lives as long as the set, a plane pool does not."""
        self._words = ("crop", cset, int(first))

    def fetch(self, extra: Optional[Sequence[torch.Tensor]] = None, with_points: bool = False):
        """ONE device-to-host wait for everything the host decides on: counters, contour counts, the first ``slots``
        contour slots of every mask (info, area / perimeter, measurement values when :meth:`launch_measure` ran, then the values of
        every family :meth:`launch` ran for, in table order whatever the launch order was) and the
        int32 device tensors in ``extra`` (returned as numpy arrays).  Falls back to the sliced copy of :meth:`host` when a
        mask has more contours than the slots fetched.  ``with_points``: the contour POINTS come over in the same copy --
        how many are in use is only known after the wait, so the copy takes as many as the previous trace of this
        ``MaskOps`` used (+ 25 %); when that was too few (the first call of a job) :meth:`records` copies them itself and
        counts it in ``blocking_point_copies``."""
        M = self.M
        k = min(self._mslots, self.C)
        parts = [self.counters, self.count, self.info[:, :k].reshape(-1)]
        f64 = [self.red[:, :k].reshape(-1)]
        if self._vals_dev is not None:
            f64.append(self._vals_dev.reshape(-1))
        live = [(self.launched[name], fam.cols) for name, fam in FAMILIES.items() if name in self.launched]
        f64 += [st.dev.reshape(-1) for st, _ in live]
        extra = list(extra or [])
        parts += [e.reshape(-1) for e in extra]
        n_pts = min(int(getattr(self.ops, "_points_hint", 0)), self.max_points) if with_points else 0
        if n_pts:
            parts.append(self.points[:n_pts].reshape(-1))
        if sum(int(t.numel()) for t in parts) % 2:            # keep the float64 block 8-byte aligned in the host copy
            parts.append(torch.zeros((1,), dtype=torch.int32, device=self.ops.device))
        ints = torch.cat(parts)
        dbl = torch.cat(f64).view(torch.int32)
        host = torch.cat([ints, dbl]).cpu().numpy()            # the wait
        pos = 0
        cnt = host[pos:pos + 4]; pos += 4
        count = host[pos:pos + M]; pos += M
        info = host[pos:pos + M * k * 4].reshape(M, k, 4); pos += M * k * 4
        outs = []
        for e in extra:
            outs.append(host[pos:pos + e.numel()].reshape(tuple(e.shape)))
            pos += e.numel()
        if with_points:
            used = int(cnt[0])
            if n_pts >= used:
                self._pts_host = host[pos:pos + 2 * used].reshape(used, 2)
            self.ops._points_hint = used + used // 4 + 4096
        d = host[int(ints.numel()):].view(np.float64)
        red = d[:M * k * 2].reshape(M, k, 2)
        if cnt[1] != 0:
            raise _lib.HipKernelError(f"contour extraction overflow (flags {int(cnt[1])}): raise max_contours / max_points")
        self.walker_stats = (int(cnt[3]), int(cnt[2]))
        mc = max(1, int(count.max()) if M else 1)
        if mc <= k:
            self.max_count = mc
            self._host = (count, info[:, :mc], red[:, :mc], int(cnt[0]))
            dpos = M * k * 2
            if self._vals_dev is not None:
                self._vals_host = d[dpos:dpos + M * k * 12].reshape(M, k, 12)[:, :mc]
                dpos += M * k * 12
            for st, cols in live:                                 # (a family launched with fewer slots than mc falls back alone)
                size = M * st.slots * cols
                st.host = d[dpos:dpos + size].reshape(M, st.slots, cols)[:, :mc] if mc <= st.slots else None
                dpos += size
        else:                                                     # a mask with many contours: the general (two-wait) path
            self._host = None
            self._vals_host = None
            for st, _ in live:
                st.host = None
            self.host()
        return outs

    def first_contour_perimeter(self) -> np.ndarray:
        """Perimeter of ``contours[0]`` (OpenCV order: the contour with the greatest (start y, start x)) per mask,
        -1 where a mask has no contour -- what ``deduplicate_masks_smart``'s compactness test reads."""
        count, info, red, _ = self.host()
        out = np.full(self.M, -1.0)
        one = count == 1                                          # the usual case: no choice to make
        out[one] = red[one, 0, 1]
        for m in np.nonzero(count > 1)[0]:
            c = int(count[m])
            k = np.lexsort((info[m, :c, 0], info[m, :c, 1]))[-1]
            out[m] = red[m, k, 1]
        return out

    def _flags(self, select: Optional[Sequence[int]]) -> Optional[torch.Tensor]:
        """[M] int32 on the device, 1 at the positions ``select``: the select of the point-table entries (None: every mask)."""
        if select is None:
            return None
        flags = np.zeros(self.M, dtype=np.int32)
        flags[np.asarray(list(select), dtype=np.int64)] = 1
        return torch.from_numpy(flags).to(self.ops.device)

    def measure(self, um_pix: float = 1.0, select: Optional[Sequence[int]] = None) -> np.ndarray:
        """[M, max contours per mask, 12] measurement values (only for the selected masks when ``select`` is given)."""
        ops = self.ops
        self.host()
        if self._vals_host is not None and self._m_um == um_pix:
            return self._vals_host                        # measured for every mask right behind the trace (launch_measure)
        M, C, mp, mc = self.M, self.C, self.max_points, self.max_count
        sel_t = self._flags(select)
        wi = torch.empty((int(ops.lib.demia_contour_work_ints(M, C, mp)),), dtype=torch.int32, device=ops.device)
        wf = torch.empty((int(ops.lib.demia_contour_work_floats(M, C, mp)),), dtype=torch.float32, device=ops.device)
        wd = torch.empty((int(ops.lib.demia_contour_work_doubles(M, C, mp)),), dtype=torch.float64, device=ops.device)
        vals = torch.zeros((M, mc, 12), dtype=torch.float64, device=ops.device)
        _lib.check(ops.lib.demia_contour_measure(_lib.ptr(sel_t), _lib.ptr(self.count), _lib.ptr(self.info), _lib.ptr(self.red),
                                                 _lib.ptr(self.points), M, C, mp, _lib.ptr(wi), _lib.ptr(wf), _lib.ptr(wd),
                                                 float(um_pix), _lib.ptr(vals), mc, ops._stream()), "demia_contour_measure")
        return vals.cpu().numpy()

    def descriptor(self, name: str, um_pix: float = 1.0, select: Optional[Sequence[int]] = None) -> np.ndarray:
        """[M, max contours per mask, cols] values of the family ``name`` of ``FAMILIES`` (only for the selected masks when ``select``
        is given: the other rows are zero).  What :meth:`launch` + :meth:`fetch` brought over, else one launch on demand over the
        contour slots in use (one more copy, as :meth:`measure`) -- a word family then reads the words where the trace's source keeps
        them (:meth:`set_plane_words` / :meth:`set_crop_words`)."""
        fam, = families((name,))
        self.host()
        st = self.launched.get(name)
        if st is not None and st.host is not None and st.um_pix == um_pix:
            return st.host                                # computed for every mask right behind the trace (launch)
        vals = torch.zeros((self.M, self.max_count, fam.cols), dtype=torch.float64, device=self.ops.device)
        fam.enqueue(self, vals, self.max_count, um_pix, None if select is None else np.asarray(list(select), dtype=np.int64))
        return vals.cpu().numpy()

    def records(self, um_pix: float = 1.0, measure: bool = True, select: Optional[Sequence[int]] = None, with_points: bool = True,
                descriptors: Sequence[str] = ()):
        """Per (selected) mask the list of contour dicts in OpenCV's order (reverse raster order of the start).  ``descriptors``: each
        dict also holds, under the name of every family named, the contour's values of :meth:`descriptor`."""
        fams = families(descriptors)
        vals = self.measure(um_pix, select) if measure else None
        desc = {fam.name: self.descriptor(fam.name, um_pix, select) for fam in fams}
        count, info, red, used = self.host()
        pts = None
        if with_points:
            if self._pts_host is not None and self._pts_host.shape[0] == used:
                pts = self._pts_host                      # came over with fetch(with_points=True): no wait of its own
            else:
                pts = self.points[:used].cpu().numpy()
                self.blocking_point_copies += 1
        out = []
        for m in (range(self.M) if select is None else select):
            recs = []
            for c in range(int(count[m])):
                sx, sy, n, off = (int(v) for v in info[m, c])
                rec = dict(start=(sx, sy), area=float(red[m, c, 0]), perimeter=float(red[m, c, 1]))
                if pts is not None:
                    rec["points"] = pts[off: off + n]             # views of this call's own host copies
                if vals is not None:
                    rec["values"] = vals[m, c]
                for name, v in desc.items():
                    rec[name] = v[m, c]
                recs.append(rec)
            if len(recs) > 1:
                recs.sort(key=lambda r: (r["start"][1], r["start"][0]), reverse=True)
            out.append(recs)
        return out
