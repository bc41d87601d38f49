"""Crop-framed mask sets: instance masks kept in the GLOBAL frame as (room, cropped packed words) instead of full-frame
planes ``[M, H, W/32]`` -- the representation of the instance tables (``demia_mask_crop_pack``, ``parallel.py``) with the HIP
kernels that COMPUTE on it (``csrc/cropops.hip``; the reading stages are ``csrc/maskops.hip``'s own kernels over
``mwords::CropWords``): tile placement, gather, the move to other rooms (``reroom``: how a set becomes an instance table,
``to_table``, and a gathered table a set again, ``from_table`` -- the exchange of the ranks without a plane), pair counts, the contour trace and the gray
histogram on the words in place (``CropMaskSet.trace`` / ``contours`` / ``gray_histogram``: ``mask_frame: crop_direct``), and the
chunked way back to planes for the plane kernels (``trace_chunks`` / ``crop_contours`` / ``crop_gray_histogram``: ``mask_frame: crop``).

All boxes are ``(y0, x0, y1, x1)``, inclusive, ``-1`` = empty -- the order every box of the C ABI has.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .maskset import (_WORKLISTS, Agglomerates, ContourSet, MaskOps, Neighbours, OutlineAgreement, PlanePool, _launch_agglomerates,
                      _launch_error_map, _launch_neighbours, _launch_outline, reads_words)
from .parallel import HDR
from .utils.mask_algebra import DeviceMaskAlgebra


def room_lengths(room: np.ndarray) -> np.ndarray:
    """Words per mask: room rows x word columns of the global word grid (0 for an empty room)."""
    room = np.asarray(room).reshape(-1, 4)
    lens = np.zeros(room.shape[0], dtype=np.int64)
    ok = room[:, 0] >= 0
    lens[ok] = (room[ok, 2].astype(np.int64) - room[ok, 0] + 1) * ((room[ok, 3] >> 5) - (room[ok, 1] >> 5) + 1)
    return lens


def room_offsets(room: np.ndarray) -> Tuple[np.ndarray, int]:
    """(exclusive prefix sums of the rooms' word counts [M] i64, total words)."""
    lens = room_lengths(room)
    offs = np.zeros(len(lens), dtype=np.int64)
    if len(lens):
        np.cumsum(lens[:-1], out=offs[1:])
    return offs, int(lens.sum())


def nearest_index(n_dst: int, n_src: int) -> np.ndarray:
    """Source index of every destination index under the placement kernels' nearest rule
    (``min(floor(t * (1 / (n_dst / n_src))), n_src - 1)`` in float64, cv2's INTER_NEAREST); non-decreasing."""
    t = np.arange(n_dst, dtype=np.float64)
    return np.minimum(np.floor(t * (1.0 / (float(n_dst) / float(n_src)))).astype(np.int64), n_src - 1)


def rooms_of_placed_tiles(boxes: np.ndarray, src_hw: Tuple[int, int], tile_hw: Tuple[int, int], x_off: Sequence[int], y_off: Sequence[int],
                          hw: Tuple[int, int]) -> np.ndarray:
    """Rooms ``[M, 4]`` i32 for ``demia_crop_place_tiles``: the boxes of tile-frame masks (``boxes``, tight or not, in the
    ``src_hw`` frame) mapped through the placement's own index rule -- every destination row / column whose source index lies
    in the box -- then pasted at the offsets and clipped to the frame ``hw``.  An upper bound of the placed masks' tight boxes
    (the tight box itself when the resize is the identity and ``boxes`` are tight), from host tables only."""
    boxes = np.asarray(boxes, dtype=np.int64).reshape(-1, 4)
    n = boxes.shape[0]
    out = np.full((n, 4), -1, dtype=np.int32)
    if n == 0:
        return out
    (sh, sw), (th, tw), (H, W) = src_hw, tile_hw, hw
    iy, ix = nearest_index(th, sh), nearest_index(tw, sw)
    xo, yo = np.asarray(x_off, dtype=np.int64), np.asarray(y_off, dtype=np.int64)
    ty0 = np.searchsorted(iy, boxes[:, 0], side="left") + yo
    ty1 = np.searchsorted(iy, boxes[:, 2], side="right") - 1 + yo
    tx0 = np.searchsorted(ix, boxes[:, 1], side="left") + xo
    tx1 = np.searchsorted(ix, boxes[:, 3], side="right") - 1 + xo
    gy0, gx0 = np.maximum(ty0, 0), np.maximum(tx0, 0)
    gy1, gx1 = np.minimum(ty1, H - 1), np.minimum(tx1, W - 1)
    ok = (boxes[:, 0] >= 0) & (gy0 <= gy1) & (gx0 <= gx1)
    out[ok] = np.stack([gy0, gx0, gy1, gx1], axis=1)[ok].astype(np.int32)
    return out


class CropMaskSet:
    """M masks over the frame ``hw = (H, W)``.

    * ``room`` [M, 4] i32: the rectangle each mask's words are stored for, columns on the global 32-bit word grid
      ``x0 >> 5 .. x1 >> 5`` exactly as ``demia_mask_crop_pack`` lays a box out (device tensor; ``room_h`` its host copy);
    * ``offsets`` [M] i64: exclusive prefix sums of rows x word columns (``offsets_h`` on the host);
    * ``payload`` i32 words; ``bbox`` [M, 4] i32 tight boxes and ``area`` [M] i32, on the device.

    Invariant: payload bits outside the tight box, and beyond column ``W - 1``, are zero.  Two sets over one frame share
    the word alignment: intersections need no bit shifts."""

    def __init__(self, ops: MaskOps, hw: Tuple[int, int], room_h: np.ndarray, payload: torch.Tensor, bbox: torch.Tensor, area: torch.Tensor,
                 room: Optional[torch.Tensor] = None, offsets: Optional[torch.Tensor] = None):
        self.ops, self.hw = ops, (int(hw[0]), int(hw[1]))
        self.room_h = np.ascontiguousarray(room_h, dtype=np.int32).reshape(-1, 4)
        self.offsets_h, self.words = room_offsets(self.room_h)
        self.payload, self.bbox, self.area = payload, bbox, area
        if room is None or offsets is None:
            if len(self):
                tab = ops.upload(np.concatenate([self.offsets_h.view(np.int32), self.room_h.reshape(-1)]))     # one copy for both
                offsets, room = tab[:2 * len(self)].view(torch.int64), tab[2 * len(self):].view(-1, 4)
            else:
                offsets = torch.zeros((0,), dtype=torch.int64, device=ops.device)
                room = torch.zeros((0, 4), dtype=torch.int32, device=ops.device)
        self.room, self.offsets = room, offsets

    def __len__(self) -> int:
        return int(self.room_h.shape[0])

    # what DeviceMaskAlgebra and the pipeline's size checks read of a plane tensor
    @property
    def shape(self) -> Tuple[int, int, int]:
        return (len(self), self.hw[0], (self.hw[1] + 31) // 32)

    @property
    def device(self):
        return self.ops.device

    @staticmethod
    def _payload(ops: MaskOps, words: int) -> torch.Tensor:
        return torch.empty((max(words, 1),), dtype=torch.int32, device=ops.device)       # (never a null pointer)

    @classmethod
    def empty(cls, ops: MaskOps, hw) -> "CropMaskSet":
        return cls(ops, hw, np.zeros((0, 4), dtype=np.int32), cls._payload(ops, 0), torch.zeros((0, 4), dtype=torch.int32, device=ops.device),
                   torch.zeros((0,), dtype=torch.int32, device=ops.device))

    # -- planes <-> crops -----------------------------------------------------------------------------------------
    @classmethod
    def from_planes(cls, ops: MaskOps, planes: torch.Tensor, W: int, bbox: Optional[np.ndarray] = None, area=None,
                    index: Optional[Sequence[int]] = None) -> "CropMaskSet":
        """Planes ``[n, H, ceil(W / 32)]`` that are zero outside their tight boxes -> a set whose rooms ARE the tight boxes
        (``demia_mask_crop_pack``).  ``bbox`` / ``area``: the tight boxes and pixel counts of all n planes when the caller has
        them on the host (a class pass does) -- else one reduction and one device-to-host wait.  ``index``: only these planes,
        in this order (no plane is copied: the others are packed as empty and left out by one gather)."""
        n, H = int(planes.shape[0]), int(planes.shape[1])
        assert planes.dtype == torch.int32 and planes.is_contiguous() and int(planes.shape[2]) == (W + 31) // 32
        if n == 0:
            return cls.empty(ops, (H, W))
        if bbox is None or area is None:
            ops.set_frame_width(W)
            a, b = ops.area_bbox(planes)
            area, bbox = a.cpu().numpy(), b.cpu().numpy()
        room_h = np.ascontiguousarray(bbox, dtype=np.int32).reshape(n, 4).copy()
        area_h = np.ascontiguousarray(area, dtype=np.int32).reshape(n)
        if index is not None:
            sel = np.asarray(index, dtype=np.int64)
            drop = np.ones(n, dtype=bool)
            drop[sel] = False
            room_h[drop] = -1
        tab = ops.upload(np.concatenate([room_h.reshape(-1), area_h]))
        bbox_d, area_d = tab[:4 * n].view(n, 4), tab[4 * n:]
        out = cls(ops, (H, W), room_h, None, bbox_d, area_d)
        out.payload = cls._payload(ops, out.words)
        if out.words:
            _lib.check(ops.lib.demia_mask_crop_pack(_lib.ptr(planes), _lib.ptr(out.room), _lib.ptr(out.offsets), n, H, W, _lib.ptr(out.payload),
                                                    ops._stream()), "demia_mask_crop_pack")
        return out if index is None else out.select(index)

    def to_planes(self, first: int = 0, n: Optional[int] = None) -> torch.Tensor:
        """Fresh zeroed planes ``[n, H, W/32]`` of the masks ``[first, first + n)`` (``demia_mask_crop_unpack``)."""
        n = len(self) - first if n is None else int(n)
        H, W = self.hw
        planes = torch.zeros((n, H, (W + 31) // 32), dtype=torch.int32, device=self.ops.device)
        if n and self.words:
            _lib.check(self.ops.lib.demia_mask_crop_unpack(_lib.ptr(self.payload), _lib.ptr(self.room[first:first + n]),
                                                           _lib.ptr(self.offsets[first:first + n]), n, H, W, _lib.ptr(planes),
                                                           self.ops._stream()), "demia_mask_crop_unpack")
        return planes

    def unpack_pooled(self, pool: PlanePool, first: int, n: int, grow: int = 0) -> torch.Tensor:
        """Masks ``[first, first + n)`` into slots ``0 .. n - 1`` of ``pool`` (``demia_crop_unpack_pooled``): the union of each
        slot's previous box and the new one is written.  Returns the view of those slots, valid until the pool is used again."""
        H, W = self.hw
        assert 0 <= first and first + n <= len(self) and pool.fits(n, H, (W + 31) // 32)
        _lib.check(self.ops.lib.demia_crop_unpack_pooled(_lib.ptr(self.payload), _lib.ptr(self.room), _lib.ptr(self.offsets), _lib.ptr(self.bbox),
                                                         int(first), int(n), H, W, _lib.ptr(pool.planes), _lib.ptr(pool.prev), int(grow),
                                                         self.ops._stream()), "demia_crop_unpack_pooled")
        return pool.planes[:n]

    # -- placement ------------------------------------------------------------------------------------------------
    @classmethod
    def place_tiles(cls, ops: MaskOps, src: torch.Tensor, room_h: np.ndarray, x_off: Sequence[int], y_off: Sequence[int], tile_h: int,
                    tile_w: int, H: int, W: int, src_w: Optional[int] = None) -> "CropMaskSet":
        """``MaskOps.place_tiles`` into rooms (``demia_crop_place_tiles``): ``room_h`` from :func:`rooms_of_placed_tiles`."""
        T, sh, swpr = (int(v) for v in src.shape)
        assert src.dtype == torch.int32 and src.is_contiguous() and len(x_off) == T and len(y_off) == T
        bbox = torch.empty((T, 4), dtype=torch.int32, device=ops.device)
        area = torch.empty((T,), dtype=torch.int32, device=ops.device)
        out = cls(ops, (H, W), room_h, None, bbox, area)
        assert len(out) == T
        out.payload = cls._payload(ops, out.words)
        if T:
            off = ops.upload(np.stack([np.asarray(x_off, dtype=np.int32), np.asarray(y_off, dtype=np.int32)]))
            _lib.check(ops.lib.demia_crop_place_tiles(_lib.ptr(src), _lib.ptr(off[0]), _lib.ptr(off[1]), T, sh, swpr * 32 if src_w is None else int(src_w),
                                                      int(tile_h), int(tile_w), H, W, _lib.ptr(out.room), _lib.ptr(out.offsets), _lib.ptr(out.payload),
                                                      _lib.ptr(area), _lib.ptr(bbox), ops._stream()), "demia_crop_place_tiles")
        return out

    # -- select / cat ---------------------------------------------------------------------------------------------
    def select(self, index: Sequence[int]) -> "CropMaskSet":
        """``self[index]`` (any order, repeats allowed) without planes: one ``demia_crop_gather``."""
        idx = np.ascontiguousarray(np.asarray(index, dtype=np.int64).reshape(-1))
        if len(idx) == 0:
            return CropMaskSet.empty(self.ops, self.hw)
        idx_d = self.ops.upload(idx)
        out = CropMaskSet(self.ops, self.hw, self.room_h[idx], None, self.bbox.index_select(0, idx_d), self.area.index_select(0, idx_d))
        out.payload = self._payload(self.ops, out.words)
        _lib.check(self.ops.lib.demia_crop_gather(_lib.ptr(self.payload), _lib.ptr(self.offsets), _lib.ptr(idx_d), _lib.ptr(out.room),
                                                  _lib.ptr(out.offsets), len(idx), _lib.ptr(out.payload), self.ops._stream()), "demia_crop_gather")
        return out

    @staticmethod
    def cat(sets: Sequence["CropMaskSet"]) -> "CropMaskSet":
        """The masks of ``sets`` (same frame) back to back: every set's words move with one ``demia_crop_gather`` into the
        result's payload."""
        sets = [s for s in sets if len(s)]
        assert sets and all(s.hw == sets[0].hw for s in sets)
        if len(sets) == 1:
            return sets[0]
        ops = sets[0].ops
        out = CropMaskSet(ops, sets[0].hw, np.concatenate([s.room_h for s in sets]), None, torch.cat([s.bbox for s in sets]),
                          torch.cat([s.area for s in sets]))
        out.payload = CropMaskSet._payload(ops, out.words)
        pos = 0
        for s in sets:
            k = len(s)
            idx = torch.arange(k, dtype=torch.int64, device=ops.device)
            _lib.check(ops.lib.demia_crop_gather(_lib.ptr(s.payload), _lib.ptr(s.offsets), _lib.ptr(idx), _lib.ptr(out.room[pos:pos + k]),
                                                 _lib.ptr(out.offsets[pos:pos + k]), k, _lib.ptr(out.payload), ops._stream()), "demia_crop_gather")
            pos += k
        return out

    # -- other rooms, instance tables ----------------------------------------------------------------------------------
    def reroom(self, room_h: np.ndarray) -> "CropMaskSet":
        """The same masks stored for the rooms ``room_h`` [M, 4] (``demia_crop_reroom``, one launch): words of a new room that lie
        in the old one are copied, the others are zero -- the same masks wherever the new room contains the tight box."""
        room_h = np.ascontiguousarray(room_h, dtype=np.int32).reshape(-1, 4)
        assert room_h.shape[0] == len(self)
        out = CropMaskSet(self.ops, self.hw, room_h, None, self.bbox, self.area)
        out.payload = self._payload(self.ops, out.words)
        if out.words:
            _lib.check(self.ops.lib.demia_crop_reroom(_lib.ptr(self.payload), _lib.ptr(self.room), _lib.ptr(self.offsets), 0, _lib.ptr(out.room),
                                                      _lib.ptr(out.offsets), len(self), int(room_lengths(room_h).max()), _lib.ptr(out.payload),
                                                      self.ops._stream()), "demia_crop_reroom")
        return out

    def tighten(self, bbox_h: np.ndarray) -> "CropMaskSet":
        """:meth:`reroom` to the tight boxes ``bbox_h`` the caller has on the host; ``self`` when the rooms already are the boxes
        (tiles that were not upscaled: the placement's rooms are exact)."""
        bbox_h = np.asarray(bbox_h, dtype=np.int32).reshape(-1, 4)
        return self if np.array_equal(self.room_h, bbox_h) else self.reroom(bbox_h)

    def to_table(self, scores: Sequence[float], classes: Sequence[int], unit_ids: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
        """The instance table of this set, ``(header [n, 10] i32, payload i32)`` on the device -- bit for bit what
        ``parallel.encode_instance_table`` makes of the same masks' planes, without a plane: the payload is the tightened set's
        words.  ONE device-to-host wait: the tight boxes and pixel counts, in a single copy."""
        n = len(self)
        hdr = np.zeros((n, HDR), dtype=np.int32)
        if n == 0:
            return torch.from_numpy(hdr).to(self.ops.device), torch.zeros((0,), dtype=torch.int32, device=self.ops.device)
        tab = torch.cat([self.bbox.reshape(-1), self.area]).cpu().numpy()
        hdr[:, 0] = np.asarray(unit_ids, dtype=np.int32)
        hdr[:, 1] = np.asarray(classes, dtype=np.int32)
        hdr[:, 2:4] = np.asarray(scores, dtype=np.float64).reshape(n, 1).view(np.int32)
        hdr[:, 4:8] = tab[:4 * n].reshape(n, 4)
        hdr[:, 8] = tab[4 * n:]
        tight = self.tighten(hdr[:, 4:8])
        return self.ops.upload(hdr), tight.payload[:tight.words]

    @staticmethod
    def table_layout(host_header: np.ndarray, offsets: Optional[np.ndarray] = None, rows: Optional[np.ndarray] = None):
        """Host arithmetic of :meth:`from_table`: (rows [k] i64, every header row's first word in the exchange buffer [n] i64, the
        words of every header row [n] i64).  Rows with box -1 (empty masks, the N4 marker) have no words."""
        hdr = np.asarray(host_header, dtype=np.int32).reshape(-1, HDR)
        lens = room_lengths(hdr[:, 4:8])
        if offsets is None:
            src_off = np.zeros(len(lens), dtype=np.int64)
            if len(lens):
                np.cumsum(lens[:-1], out=src_off[1:])
        else:
            src_off = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        assert len(src_off) == len(lens)
        rows = np.arange(len(lens), dtype=np.int64) if rows is None else np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
        return rows, src_off, lens

    @classmethod
    def from_table(cls, ops: MaskOps, hw: Tuple[int, int], host_header: np.ndarray, payload: torch.Tensor, offsets: Optional[np.ndarray] = None,
                   rows: Optional[np.ndarray] = None) -> "CropMaskSet":
        """The set of the rows ``rows`` (default: all, in order) of an instance table whose header is on the host
        (``GlobalTable.host_header``): rooms, boxes and pixel counts are the header's, the words come out of the exchange buffer
        ``payload`` where ``offsets`` (``GlobalTable.offsets``; default: back to back in header order) says they are -- one
        ``demia_crop_reroom`` with the rows as its index, no plane and no wait."""
        hdr = np.asarray(host_header, dtype=np.int32).reshape(-1, HDR)
        rows, src_off, lens = cls.table_layout(hdr, offsets, rows)
        k = len(rows)
        if k == 0:
            return cls.empty(ops, hw)
        n = hdr.shape[0]
        assert payload.dtype == torch.int32 and payload.is_contiguous() and payload.is_cuda
        # (the kernel reads what these tables say: every listed row's words must lie inside the buffer)
        assert rows.min() >= 0 and rows.max() < n and src_off.min() >= 0 and int((src_off + lens).max()) <= payload.numel()
        tab = ops.upload(np.concatenate([hdr[:, 4:8].reshape(-1), src_off.view(np.int32), rows.view(np.int32), hdr[rows, 8]]))     # one copy
        src_room_d, src_off_d = tab[:4 * n].view(n, 4), tab[4 * n:6 * n].view(torch.int64)
        rows_d, area_d = tab[6 * n:6 * n + 2 * k].view(torch.int64), tab[6 * n + 2 * k:]
        out = cls(ops, hw, hdr[rows, 4:8], None, None, area_d)
        out.bbox = out.room                                                       # (a table's rooms ARE the tight boxes)
        out.payload = cls._payload(ops, out.words)
        if out.words:
            _lib.check(ops.lib.demia_crop_reroom(_lib.ptr(payload), _lib.ptr(src_room_d), _lib.ptr(src_off_d), _lib.ptr(rows_d), _lib.ptr(out.room),
                                                 _lib.ptr(out.offsets), k, int(lens[rows].max()), _lib.ptr(out.payload), ops._stream()),
                       "demia_crop_reroom")
        return out

    def host_crops(self):
        """Per mask its room's crop on the host: ``(y0, x0, bool[h, w])`` or ``None`` for an empty room (what ``mask_crops``
        returns of planes, with the room in place of the tight box: the same pixels are set)."""
        pay = self.payload[:self.words].cpu().numpy().view(np.uint32)
        out = []
        for (y0, x0, y1, x1), off in zip(self.room_h.tolist(), self.offsets_h.tolist()):
            if y0 < 0:
                out.append(None)
                continue
            rows, c0, cols = y1 - y0 + 1, x0 >> 5, (x1 >> 5) - (x0 >> 5) + 1
            words = np.ascontiguousarray(pay[off: off + rows * cols].reshape(rows, cols))
            bits = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")
            out.append((y0, x0, bits[:, x0 - 32 * c0: x1 - 32 * c0 + 1].astype(bool)))
        return out

    # -- pair counts ----------------------------------------------------------------------------------------------
    def pair_matrix(self, first: np.ndarray, count: np.ndarray, label: Optional[np.ndarray] = None, ld: Optional[int] = None) -> torch.Tensor:
        """``MaskOps.pair_matrix`` on the cropped words (``demia_crop_pair_matrix``): same segments, same ``[M, ld]`` layout."""
        M, ops = len(self), self.ops
        if ld is None:
            ld = max(1, int(np.max(count)) if M else 1)
        out = torch.zeros((M, ld), dtype=torch.int32, device=ops.device)
        if M == 0:
            return out
        tab = np.stack([np.asarray(first, dtype=np.int32), np.asarray(count, dtype=np.int32),
                        np.asarray(label if label is not None else np.zeros(M), dtype=np.int32)])
        tt = ops.upload(tab)
        _lib.check(ops.lib.demia_crop_pair_matrix(_lib.ptr(self.payload), _lib.ptr(self.room), _lib.ptr(self.offsets), _lib.ptr(self.bbox),
                                                  _lib.ptr(tt[0]), _lib.ptr(tt[1]), _lib.ptr(tt[2]) if label is not None else 0, _lib.ptr(out), M, ld,
                                                  ops._stream()), "demia_crop_pair_matrix")
        return out

    def pair_intersections(self, other: "CropMaskSet", pi: np.ndarray, pj: np.ndarray) -> np.ndarray:
        """``|self[pi[p]] & other[pj[p]]|`` per listed pair (``demia_crop_pair_intersections``); one device-to-host wait."""
        P, ops = len(pi), self.ops
        if P == 0:
            return np.zeros((0,), dtype=np.int64)
        assert self.hw == other.hw
        tp = ops.upload(np.stack([np.asarray(pi, dtype=np.int32), np.asarray(pj, dtype=np.int32)]))
        out = torch.empty((P,), dtype=torch.int32, device=ops.device)
        _lib.check(ops.lib.demia_crop_pair_intersections(_lib.ptr(self.payload), _lib.ptr(self.room), _lib.ptr(self.offsets), _lib.ptr(self.bbox),
                                                         _lib.ptr(other.payload), _lib.ptr(other.room), _lib.ptr(other.offsets), _lib.ptr(other.bbox),
                                                         _lib.ptr(tp[0]), _lib.ptr(tp[1]), _lib.ptr(out), P, ops._stream()),
                   "demia_crop_pair_intersections")
        return out.cpu().numpy().astype(np.int64)

    # -- contours, measurements, histogram on the words in place ----------------------------------------------------------
    def contour_scratch(self) -> Tuple[np.ndarray, int]:
        """(``scratch_off`` [M] i64, total u32 words) of the scratch a trace of this set needs (``demia_crop_contour_scratch``): host
        tables only; non-zero for the masks whose room's region exceeds the trace's large LDS buffer."""
        M = len(self)
        off = np.zeros(max(M, 1), dtype=np.int64)
        total = int(self.ops.lib.demia_crop_contour_scratch(self.room_h.ctypes.data, M, self.hw[0], self.hw[1], off.ctypes.data))
        return off[:M], total

    def _lazy_scratch(self, key: str, sizer) -> Tuple[torch.Tensor, torch.Tensor]:
        """(scratch words, ``scratch_off`` [M] i64) on the device, sized by ``sizer() -> (offsets on the host, total words)`` and
        made on first use: a set nobody asks stays without them."""
        got = self.__dict__.get(key)
        if got is None:
            off_h, total = sizer()
            if total:
                got = (torch.empty((total,), dtype=torch.int32, device=self.ops.device), self.ops.upload(off_h))
            else:
                t = torch.empty((2,), dtype=torch.int32, device=self.ops.device)      # (never read)
                got = (t, t)
            self.__dict__[key] = got
        return got

    def inscribed_scratch(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """The scratch of the word entries (``demia_crop_inscribed``, ``demia_crop_skeleton``) over masks of this set, sized by
        :meth:`contour_scratch` -- the tracer's contract."""
        return self._lazy_scratch("_insc_scratch", self.contour_scratch)

    def skeleton_scratch(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """The second scratch of ``demia_crop_skeleton`` over masks of this set, sized from the rooms alone
        (``demia_crop_skeleton_scratch``: one more padded room region per mask whose region exceeds the large LDS buffer)."""
        def sizer():
            M = len(self)
            off = np.zeros(max(M, 1), dtype=np.int64)
            total = int(self.ops.lib.demia_crop_skeleton_scratch(self.room_h.ctypes.data, M, self.hw[0], self.hw[1], off.ctypes.data))
            return off[:M], total
        return self._lazy_scratch("_skel_scratch", sizer)

    def boundary_band(self, d: int, bbox: Optional[torch.Tensor] = None) -> "CropMaskSet":
        """The boundary bands ``m & ~eroded(m, d)`` of the set's masks as a set over the SAME rooms (``demia_crop_boundary_band``; the
        definition is in ``include/deepemia_hip.h``): its ``area`` holds the band pixel counts, its ``bbox`` the masks' tight boxes
        (a band has its mask's).  Enqueued without a wait; this set is left as it is.  ``bbox``: the tight boxes on the device
        when the caller has its own copy (default: the set's)."""
        ops, M = self.ops, len(self)
        d = int(d)
        if d < 1:
            raise ValueError(f"boundary_band: d must be an integer >= 1, got {d}")
        if M == 0:
            return CropMaskSet.empty(ops, self.hw)
        bbox = self.bbox if bbox is None else bbox
        payload = torch.zeros((max(self.words, 1),), dtype=torch.int32, device=ops.device)
        area = torch.zeros((M,), dtype=torch.int32, device=ops.device)

        def sizer():
            off = np.zeros(max(M, 1), dtype=np.int64)
            total = int(ops.lib.demia_crop_boundary_scratch(self.room_h.ctypes.data, M, self.hw[0], self.hw[1], off.ctypes.data))
            return off[:M], total
        scratch, scratch_off = self._lazy_scratch("_band_scratch", sizer)
        _lib.check(ops.lib.demia_crop_boundary_band(_lib.ptr(self.payload), _lib.ptr(self.room), _lib.ptr(self.offsets), _lib.ptr(bbox), M,
                                                    self.hw[0], self.hw[1], d, _lib.ptr(payload), _lib.ptr(area), _lib.ptr(scratch),
                                                    _lib.ptr(scratch_off), ops._stream()), "demia_crop_boundary_band")
        return CropMaskSet(ops, self.hw, self.room_h, payload, bbox, area, room=self.room, offsets=self.offsets)

    def outline_agreement(self, gt: "CropMaskSet", pairs, area=None, gt_area=None, bbox: Optional[torch.Tensor] = None) -> OutlineAgreement:
        """``MaskOps.outline_agreement`` of this set (the detections) against ``gt`` (the annotations) over the same frame, on the
        words in place (``demia_crop_outline_agreement``): the same records, no plane, no wait.  ``area`` / ``gt_area``: the pixel
        counts on the host; None: the sets' own are read with a wait of their own (callers outside the evaluate task).  ``bbox``:
        this set's tight boxes on the device when the caller has its own copy (default: the set's)."""
        ops, D, G = self.ops, len(self), len(gt)
        if self.hw != gt.hw:
            raise ValueError(f"outline_agreement: a set over {self.hw} against a set over {gt.hw}")
        if area is None:
            area = self.area.cpu().numpy() if D else np.zeros(0)
        if gt_area is None:
            gt_area = gt.area.cpu().numpy() if G else np.zeros(0)
        return _launch_outline(ops, "demia_crop_outline_agreement", (self.payload, self.room, self.offsets, self.bbox if bbox is None else bbox),
                               D, area, (gt.payload, gt.room, gt.offsets, gt.bbox), G, gt_area, self.hw[0], self.hw[1], pairs)

    def error_map(self, gt: "CropMaskSet", d_state, g_state, image: torch.Tensor, alpha: int, line: int, palette=None,
                  bbox: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """``MaskOps.error_map`` of this set (the detections) against ``gt`` (the annotations) over the same frame, on the words in
        place (``demia_crop_error_map``): the same picture and counts, no plane, no wait -- the image and its painted copy are the
        only full-frame buffers.  ``bbox``: this set's tight boxes on the device when the caller has its own copy (default: the
        set's)."""
        if self.hw != gt.hw:
            raise ValueError(f"error_map: a set over {self.hw} against a set over {gt.hw}")
        return _launch_error_map(self.ops, "demia_crop_error_map", (self.payload, self.room, self.offsets, self.bbox if bbox is None else bbox),
                                 len(self), d_state, (gt.payload, gt.room, gt.offsets, gt.bbox), len(gt), g_state, self.hw[0], self.hw[1],
                                 image, alpha, line, palette)

    def trace(self, max_contours: int = 64, max_points: Optional[int] = None, total_area=None, scratch: Optional[torch.Tensor] = None,
              keep_words: bool = False) -> ContourSet:
        """``MaskOps.trace`` over ALL masks of the set, read where they are (``demia_crop_contours_wl``): no plane, no chunk, no
        wait.  The point pool is sized as ``MaskOps.trace`` sizes it from ``total_area`` (the masks' pixel count, or counts, on the
        host), else from the mask count as ``trace_chunks`` does -- a caller that meets an overflow traces again with the areas.
        ``scratch``: the caller's own i32 words, at least :meth:`contour_scratch`'s total (default: allocated here).
        ``keep_words``: the contour set remembers this set as the source of its words (the word families of ``FAMILIES``)."""
        ops, M = self.ops, len(self)
        H, W = self.hw
        if max_points is None:
            if total_area is not None:
                max_points = int(min(max(4 * int(np.sum(total_area)) // 8 + 4096 * M, 1 << 16), 1 << 26))
            else:
                max_points = int(min(4096 * M + (1 << 16), 1 << 26))
        cs = ContourSet(ops, M, int(max_contours), max_points)
        if keep_words:
            cs.set_crop_words(self, 0)
        if M == 0:
            return cs
        off_h, total = self.contour_scratch()
        if total:
            off_d = ops.upload(off_h)
            if scratch is None:
                scratch = torch.empty((total,), dtype=torch.int32, device=ops.device)
            assert scratch.dtype == torch.int32 and scratch.is_contiguous() and scratch.numel() >= total
        else:
            scratch = off_d = torch.empty((1,), dtype=torch.int32, device=ops.device) if scratch is None else scratch      # (never read)
        worklist = torch.empty((M + 2,), dtype=torch.int32, device=ops.device) if _WORKLISTS else None
        _lib.check(ops.lib.demia_crop_contours_wl(_lib.ptr(self.payload), _lib.ptr(self.room), _lib.ptr(self.offsets), _lib.ptr(self.bbox), M, H, W,
                                                  cs.C, max_points, _lib.ptr(cs.count), _lib.ptr(cs.info), _lib.ptr(cs.red), _lib.ptr(cs.points),
                                                  _lib.ptr(cs.counters), _lib.ptr(worklist), _lib.ptr(scratch), _lib.ptr(off_d), ops._stream()),
                   "demia_crop_contours_wl")
        return cs

    def contours(self, max_contours: int = 64, max_points: Optional[int] = None, um_pix: float = 1.0, measure: bool = True, total_area=None,
                 extra: Optional[Sequence[torch.Tensor]] = None, descriptors: Sequence[str] = ()):
        """``MaskOps.contours`` for this set: one trace, the measurements of every mask's first four contours right behind it, ONE
        fetch (``extra`` rides on it); same records, same return value.  Without ``total_area`` the point pool is sized from the
        mask count; if it overflows, the set is traced again with the pool sized from its own (device) areas -- one more wait.
        ``descriptors``: the records also carry the named families of ``FAMILIES`` (``ContourSet.launch``), in that same fetch; the
        word families read the words in place."""
        keep_words = reads_words(descriptors)
        if len(self) == 0:
            return [] if extra is None else ([], [e.cpu().numpy() for e in extra])

        def run(area):
            cs = self.trace(max_contours, max_points, total_area=area, keep_words=keep_words)
            cs.launch_all(um_pix, measure, descriptors, slots=4)
            return cs, cs.fetch(extra=extra, with_points=True)
        try:
            cs, got = run(total_area)
        except _lib.HipKernelError as e:
            if "overflow" not in str(e) or total_area is not None or max_points is not None:
                raise
            cs, got = run(int(self.area.sum().item()))
        recs = cs.records(um_pix=um_pix, measure=measure, descriptors=descriptors)
        return recs if extra is None else (recs, list(got))

    def neighbours(self, area=None, group=None, r2: int = -1) -> Neighbours:
        """``MaskOps.neighbours`` on the words in place (``demia_crop_neighbours``): the same tables, no plane, no wait.  ``area``:
        the pixel counts on the host; None: the set's own are read with a wait of their own (callers outside the pipeline)."""
        M, ops = len(self), self.ops
        H, W = self.hw
        if area is None:
            area = self.area.cpu().numpy() if M else np.zeros(0)
        return _launch_neighbours(ops, "demia_crop_neighbours", (self.payload, self.room, self.offsets, self.bbox), M, H, W, area, group, r2)

    def agglomerates(self, area=None, group=None, l2: int = 2, border: Optional[Neighbours] = None, label_lds_cap: int = 0) -> Agglomerates:
        """``MaskOps.agglomerates`` on the words in place (``demia_crop_agglomerates``): the same tensors, no plane, no wait.
        ``area``: the pixel counts on the host; None (and no ``border``): the set's own are read with a wait of their own.
        ``border``: the ``Neighbours`` of :meth:`neighbours` on this set, whose border points are reused."""
        M, ops = len(self), self.ops
        H, W = self.hw
        if area is None and border is None:
            area = self.area.cpu().numpy() if M else np.zeros(0)
        return _launch_agglomerates(ops, "demia_crop_agglomerates", (self.payload, self.room, self.offsets, self.bbox), M, H, W, area, group,
                                    l2, border, label_lds_cap)

    def gray_histogram(self, image: torch.Tensor) -> np.ndarray:
        """``MaskOps.gray_histogram`` on the words in place (``demia_crop_gray_histogram``): [M, 256] gray-level counts."""
        M, ops = len(self), self.ops
        if M == 0:
            return np.zeros((0, 256), dtype=np.int64)
        H, W = self.hw
        assert image.dtype == torch.uint8 and image.is_contiguous() and tuple(image.shape[:2]) == (H, W), (image.shape, H, W)
        ch = 1 if image.dim() == 2 else int(image.shape[2])
        hist = torch.empty((M, 256), dtype=torch.int32, device=ops.device)
        _lib.check(ops.lib.demia_crop_gray_histogram(_lib.ptr(self.payload), _lib.ptr(self.room), _lib.ptr(self.offsets), _lib.ptr(self.bbox),
                                                     _lib.ptr(image), ch, M, H, W, _lib.ptr(hist), ops._stream()), "demia_crop_gray_histogram")
        return hist.cpu().numpy().astype(np.int64)


class CropMaskAlgebra(DeviceMaskAlgebra):
    """:class:`DeviceMaskAlgebra` over a :class:`CropMaskSet`: boxes and pixel counts are the set's own (``area`` / ``bbox``: their
    host copies when the caller has them -- nothing is uploaded or fetched then), and every count the base class asks of the
    device goes through :meth:`intersections`, i.e. ``demia_crop_pair_intersections`` -- the one place of the base class that
    reads ``self.packed`` (``inter_row``, ``prefetch_overlapping_pairs`` and ``inter`` all end there)."""

    def __init__(self, cset: CropMaskSet, area=None, bbox=None, blocks=None):
        super().__init__(cset.ops, cset, area=cset.area if area is None else area, bbox=cset.bbox if bbox is None else bbox, blocks=blocks,
                         bbox_dev=cset.bbox)

    def intersections(self, pi, pj) -> np.ndarray:
        pi = np.asarray(pi, dtype=np.int64)
        pj = np.asarray(pj, dtype=np.int64)
        out = self.packed.pair_intersections(self.packed, pi, pj)
        for a, b, v in zip(pi.tolist(), pj.tolist(), out.tolist()):
            self._cache[(a, b)] = v
            self._cache[(b, a)] = v
        self.I[pi, pj] = out
        self.I[pj, pi] = out
        self.known[pi, pj] = True
        self.known[pj, pi] = True
        return out


class CropPlanes:
    """The full-frame planes a crop-framed image ever holds: a :class:`PlanePool` of ``chunk`` planes the masks are unpacked
    into, ``chunk`` masks at a time, plus as many scratch planes for the kernels that want them (the contour trace's regions
    that do not fit in LDS).  ``cap`` = all of them: 32 planes -- 4 MiB of a 1024^2 frame, 256 MiB of an 8192^2 frame."""

    CHUNK = 16

    def __init__(self, ops: MaskOps, hw: Tuple[int, int], chunk: int = CHUNK):
        H, W = int(hw[0]), int(hw[1])
        wpr = (W + 31) // 32
        self.hw, self.chunk, self.cap = (H, W), int(chunk), 2 * int(chunk)
        self.pool = PlanePool(ops.device, H, wpr, self.chunk)
        self.scratch = torch.empty((self.chunk, H, wpr), dtype=torch.int32, device=ops.device)


def crop_planes(ops: MaskOps, hw: Tuple[int, int]) -> CropPlanes:
    """The :class:`CropPlanes` of this ``MaskOps`` (one per host thread) for the frame ``hw``, reallocated when the frame changes."""
    cp = ops.__dict__.get("_crop_planes")
    if cp is None or cp.hw != (int(hw[0]), int(hw[1])):
        ops.__dict__.pop("_crop_planes", None)
        cp = ops.__dict__["_crop_planes"] = CropPlanes(ops, hw)
    return cp


def _trace_chunk(cset: CropMaskSet, planes: CropPlanes, f: int, n: int, max_contours: int, um_pix: Optional[float], descriptors: Sequence[str],
                 **pool_size) -> ContourSet:
    """Masks ``[f, f + n)`` of ``cset`` unpacked into the pool and traced there, with the 12 measurements and the families
    ``descriptors`` enqueued behind the trace when ``um_pix`` is given; nothing is waited for.  ``pool_size``: ``max_points`` or
    ``total_area`` of ``MaskOps.trace``.  A word family makes the contour set remember ``cset`` and ``f`` as the source of its
    words: it reads the set's PAYLOAD -- at the launch here and on demand later -- never the pool, which the next chunk overwrites."""
    pl = cset.unpack_pooled(planes.pool, f, n)
    cs = cset.ops.trace(pl, max_contours=max_contours, bbox=cset.bbox[f:f + n], scratch=planes.scratch[:n], **pool_size)
    if reads_words(descriptors):
        cs.set_crop_words(cset, f)
    if um_pix is not None:
        cs.launch_all(um_pix, True, descriptors, slots=4)
    return cs


def trace_chunks(cset: CropMaskSet, planes: CropPlanes, max_contours: int = 256, um_pix: Optional[float] = None,
                 total_area: Optional[np.ndarray] = None, descriptors: Sequence[str] = ()):
    """The contour trace of every mask of ``cset`` (``MaskOps.trace``, unchanged), ``planes.chunk`` masks at a time through the
    pool: yields (first, n, ContourSet) per chunk, each with its unpack + trace (+ the measurements of its first contours when
    ``um_pix`` is given) enqueued and NOT waited for, and with the NEXT chunk already enqueued behind it -- the pool is reused
    in stream order, every chunk's contour tables are its own -- so the consumer's fetch of one chunk overlaps the device's
    work on the next, and the contour tables of two chunks at most are alive.  ``total_area``: the masks' pixel counts when
    they are on the host -- sizes every chunk's point pool as ``MaskOps.trace`` does (else from the mask count; a caller that
    meets an overflow traces that chunk again).  ``descriptors``: with ``um_pix``, the named families of ``FAMILIES`` are enqueued
    behind the measurements (``ContourSet.launch_all``)."""
    reads_words(descriptors)                # (an unknown name raises for an empty set too)
    cset.ops.set_frame_width(cset.hw[1])
    pending = None
    for f in range(0, len(cset), planes.chunk):
        n = min(planes.chunk, len(cset) - f)
        if total_area is not None:
            mp = int(min(max(4 * int(np.sum(total_area[f:f + n])) // 8 + 4096 * n, 1 << 16), 1 << 26))
        else:
            mp = int(min(4096 * n + (1 << 16), 1 << 26))
        cs = _trace_chunk(cset, planes, f, n, max_contours, um_pix, descriptors, max_points=mp)
        if pending is not None:
            yield pending
        pending = (f, n, cs)
    if pending is not None:
        yield pending


def crop_contours(cset: CropMaskSet, planes: CropPlanes, um_pix: float = 1.0, total_area: Optional[np.ndarray] = None,
                  extra: Optional[Sequence[torch.Tensor]] = None, max_contours: int = 256, descriptors: Sequence[str] = ()):
    """``MaskOps.contours`` (trace + the 12 measurements, records in OpenCV's order) for a crop-framed set, chunk by chunk
    through the plane pool.  ``extra``: int32 device tensors that come to the host with the FIRST chunk's tables.
    ``total_area``: the masks' pixel counts on the host (sizes the point pools); without them the pools are sized from the mask
    count, and a chunk whose pool overflows is unpacked and traced again with the pool sized from its own (device) areas.
    ``descriptors``: the records also carry the named families of ``FAMILIES``, in each chunk's one fetch.
    Returns (records per mask, host arrays of ``extra`` or None); one device-to-host wait per chunk."""
    area = None if total_area is None else np.asarray(total_area).reshape(-1)
    recs, got = [], None
    for k, (f, n, cs) in enumerate(trace_chunks(cset, planes, max_contours, um_pix=um_pix, total_area=area, descriptors=descriptors)):
        ex = extra if k == 0 else None
        try:
            g = cs.fetch(extra=ex, with_points=True)
        except _lib.HipKernelError as e:
            if "overflow" not in str(e):
                raise
            # (the chunk behind this one has run: the pool is free again)
            cs = _trace_chunk(cset, planes, f, n, max_contours, um_pix, descriptors, total_area=int(cset.area[f:f + n].sum().item()))
            g = cs.fetch(extra=ex, with_points=True)
        if k == 0:
            got = list(g)
        recs.extend(cs.records(um_pix=um_pix, measure=True, descriptors=descriptors))
    if extra is not None and got is None:
        got = [e.cpu().numpy() for e in extra]
    return recs, (got if extra is not None else None)


def crop_gray_histogram(cset: CropMaskSet, planes: CropPlanes, image: torch.Tensor) -> np.ndarray:
    """``MaskOps.gray_histogram`` for a crop-framed set, chunk by chunk through the plane pool: [M, 256] gray-level counts."""
    out = [np.zeros((0, 256), dtype=np.int64)]
    cset.ops.set_frame_width(cset.hw[1])
    for f in range(0, len(cset), planes.chunk):
        n = min(planes.chunk, len(cset) - f)
        out.append(cset.ops.gray_histogram(cset.unpack_pooled(planes.pool, f, n), image, bbox=cset.bbox[f:f + n]))
    return np.concatenate(out)
