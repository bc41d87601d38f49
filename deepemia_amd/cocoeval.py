"""COCO box / mask AP for the evaluate task: pycocotools' ``COCOeval`` (``useCats=1``) and the mask codecs it relies on,
with the per-pixel and per-pair work on the MI355X and the greedy matching in native host code.

Device (``csrc/evaluate.hip``): polygon rasterisation with ``rleFrPoly``'s rule (``rasterize_polygons``), the detection x
ground-truth intersection matrix of one image (``cross_matrix``), column-major run lengths of packed masks
(``rle_counts``) -- each on full-frame planes and, with the ``_crop`` suffix, on crop-framed sets (:class:`CropMaskSet`: rooms,
never planes; the same kernels over another word source).  Host native (``csrc/hostloops.hip``): ``evaluateImg`` for every (task, category, image, area range, IoU
threshold) in one call (``match``) and ``rleToString`` (``rle_strings``).  numpy: the IoU tables, ``accumulate`` and
``summarize``.
"""
from __future__ import annotations

import csv
import ctypes as C
import os
from functools import partial
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .cropset import CropMaskSet, room_lengths

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = [1, 10, 100]
AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], dtype=np.float64)
AREA_LBL = ["all", "small", "medium", "large"]
METRICS = ["AP", "AP50", "AP75", "APs", "APm", "APl"]


def _ptr(a: np.ndarray) -> int:
    return 0 if a is None or a.size == 0 else a.ctypes.data


# ---- device ----------------------------------------------------------------------------------------------------------------
class _PolygonTables:
    """The host tables of the rasteriser for ``masks[m]`` = the polygons of mask m, uploaded: vertices, the polygon and vertex
    index of every edge, the polygons of every mask, the room of every polygon's boundary points, and the zeroed counters with
    the error word behind them."""

    def __init__(self, ops, masks):
        verts, vert_off, mask_poly = [], [0], [0]
        for polys in masks:
            for p in polys:
                a = np.asarray(p, dtype=np.float64).reshape(-1, 2)
                verts.append(a)
                vert_off.append(vert_off[-1] + len(a))
            mask_poly.append(len(vert_off) - 1)
        xy = np.ascontiguousarray(np.concatenate(verts) if verts else np.zeros((0, 2)), dtype=np.float64)
        vo = np.asarray(vert_off, dtype=np.int64)
        k = np.diff(vo)
        P, E = len(k), int(vo[-1])
        edge_poly = np.repeat(np.arange(P), k)
        edge_idx = np.arange(E) - np.repeat(vo[:-1], k)
        nxt = np.where(edge_idx + 1 == np.repeat(k, k), np.repeat(vo[:-1], k), np.arange(E) + 1)
        # room for the kept boundary points: at most one per walk point, max(|dx|, |dy|) + 1 of the x5 lattice per edge
        span = np.abs(xy[nxt] - xy[np.arange(E)]).max(axis=1) if E else np.zeros((0,))
        room = np.floor(5.0 * span).astype(np.int64) + 3
        bnd_off = np.zeros(P + 1, dtype=np.int64)
        np.cumsum(np.bincount(edge_poly, weights=room, minlength=P).astype(np.int64), out=bnd_off[1:])
        tab = np.concatenate([vo.astype(np.int32), edge_poly.astype(np.int32), edge_idx.astype(np.int32),
                              np.asarray(mask_poly, dtype=np.int32)])
        self.P, self.E = P, E
        self.t_tab = torch.from_numpy(tab).to(ops.device)
        self.t_xy = torch.from_numpy(xy if len(xy) else np.zeros((1, 2))).to(ops.device)
        self.t_off = torch.from_numpy(bnd_off).to(ops.device)
        self.bnd = torch.empty((max(1, int(bnd_off[-1])), 2), dtype=torch.int32, device=ops.device)
        self.cnt = torch.zeros((P + 1,), dtype=torch.int32, device=ops.device)           # [P] counters + the error word
        self.err = self.cnt[P:]

    def args(self):
        """The arguments that ``demia_poly_rasterize`` and ``demia_crop_poly_rasterize`` share, up to ``mask_poly``."""
        P, E, t = self.P, self.E, self.t_tab
        o_e, o_i, o_m = P + 1, P + 1 + E, P + 1 + 2 * E
        return (_lib.ptr(self.t_xy), _lib.ptr(t), _lib.ptr(t[o_e:]) if E else _lib.ptr(t), _lib.ptr(t[o_i:]) if E else _lib.ptr(t),
                _lib.ptr(self.t_off), _lib.ptr(self.bnd), _lib.ptr(self.cnt), _lib.ptr(self.err), E, _lib.ptr(t[o_m:]))


def rasterize_polygons(ops, masks: Sequence[Sequence[Sequence[float]]], H: int, W: int, err_out: Optional[list] = None
                       ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``masks[m]`` = the polygons of mask m, each a flat ``[x0, y0, x1, y1, ...]`` list -> packed ``[M, H, ceil(W/32)]`` int32
    on the device, pixel count ``[M]`` and tight box ``[M, 4]`` (``demia_poly_rasterize``).  The kernel's error word is waited
    for and checked here, unless ``err_out`` is a list: the word (a 1-element device tensor) is then appended to it for the
    caller to fetch with its own tables and hand to :func:`check_rasterize_error`."""
    M = len(masks)
    wpr = (W + 31) // 32
    out = torch.empty((M, H, wpr), dtype=torch.int32, device=ops.device)
    area = torch.empty((M,), dtype=torch.int32, device=ops.device)
    bbox = torch.empty((M, 4), dtype=torch.int32, device=ops.device)
    if M == 0:
        return out, area, bbox
    tabs = _PolygonTables(ops, masks)
    _lib.check(ops.lib.demia_poly_rasterize(*tabs.args(), M, H, W, _lib.ptr(out), _lib.ptr(area), _lib.ptr(bbox), ops._stream()),
               "demia_poly_rasterize")
    if err_out is not None:
        err_out.append(tabs.err)
    else:
        check_rasterize_error(int(tabs.err[0].item()))
    return out, area, bbox


def polygon_rooms(masks: Sequence[Sequence[Sequence[float]]], H: int, W: int) -> np.ndarray:
    """The rooms ``[M, 4]`` i32 (y0, x0, y1, x1, -1 = empty) that :func:`rasterize_polygons_crop` stores the masks for, from the
    vertices alone (host arithmetic, nothing is waited for): columns ``max(0, floor(min x) - 1) .. min(W - 1, ceil(max x))``,
    rows ``max(0, floor(min y) - 1) .. min(H - 1, ceil(max y))`` over all vertices of the mask's polygons, empty when that
    rectangle is.  ``rleFrPoly`` rounds a vertex to the nearest fifth of a pixel and sets pixel centres, so no set pixel lies
    more than one pixel outside the vertices' hull; the rasteriser's error word reports a mask this rule would not hold."""
    out = np.full((len(masks), 4), -1, dtype=np.int32)
    for m, polys in enumerate(masks):
        pts = [np.asarray(p, dtype=np.float64).reshape(-1, 2) for p in polys]
        pts = np.concatenate(pts) if pts else np.zeros((0, 2))
        if len(pts) == 0 or not np.isfinite(pts).all():
            continue
        lo, hi = np.floor(pts.min(axis=0)) - 1, np.ceil(pts.max(axis=0))
        x0, y0 = int(max(0.0, lo[0])) if lo[0] < W else W, int(max(0.0, lo[1])) if lo[1] < H else H
        x1, y1 = int(min(float(W - 1), hi[0])) if hi[0] >= 0 else -1, int(min(float(H - 1), hi[1])) if hi[1] >= 0 else -1
        if x0 <= x1 and y0 <= y1:
            out[m] = (y0, x0, y1, x1)
    return out


def rasterize_polygons_crop(ops, masks: Sequence[Sequence[Sequence[float]]], H: int, W: int, rooms: Optional[np.ndarray] = None
                            ) -> Tuple[CropMaskSet, torch.Tensor]:
    """:func:`rasterize_polygons` into the rooms of a :class:`CropMaskSet` (``demia_crop_poly_rasterize``): the same bits, the
    pixel counts and the tight boxes, and no ``[M, H, wpr]`` tensor.  ``rooms`` default to :func:`polygon_rooms`.  Nothing is
    waited for: the second value is the kernel's error word (a 1-element device tensor) for the caller to fetch with its own
    tables and hand to :func:`check_rasterize_error`."""
    M = len(masks)
    if M == 0:
        return CropMaskSet.empty(ops, (H, W)), torch.zeros((1,), dtype=torch.int32, device=ops.device)
    room_h = polygon_rooms(masks, H, W) if rooms is None else np.ascontiguousarray(rooms, dtype=np.int32).reshape(M, 4)
    area = torch.empty((M,), dtype=torch.int32, device=ops.device)
    bbox = torch.empty((M, 4), dtype=torch.int32, device=ops.device)
    out = CropMaskSet(ops, (H, W), room_h, None, bbox, area)
    out.payload = CropMaskSet._payload(ops, out.words)
    tabs = _PolygonTables(ops, masks)
    _lib.check(ops.lib.demia_crop_poly_rasterize(*tabs.args(), M, H, W, _lib.ptr(out.room), _lib.ptr(out.offsets),
                                                 int(room_lengths(room_h).max()), _lib.ptr(out.payload), _lib.ptr(area), _lib.ptr(bbox),
                                                 ops._stream()), "demia_crop_poly_rasterize")
    return out, tabs.err


def check_rasterize_error(word: int) -> None:
    """Raise for the rasteriser's error word: bit 1 = a boundary list overflowed, bit 2 (rooms only) = a mask's boundary points
    could set a pixel outside its room."""
    if word & 1:
        raise _lib.HipKernelError("demia_poly_rasterize: a boundary list overflowed its room")
    if word:
        raise _lib.HipKernelError("demia_crop_poly_rasterize: a polygon's boundary points reach outside its mask's room")


def rle_host_crop(counts: Sequence[int], H: int, W: int):
    """Run lengths (background first, column-major, as ``rle_decode`` takes them) -> ``(box (y0, x0, y1, x1), words uint32, pixel
    count)`` on the host: the tight box from the runs, then the box's rows packed in the layout of a room (rows x word columns
    ``x0 >> 5 .. x1 >> 5``).  Only the box's columns are ever dense; an empty mask gives ``((-1,) * 4, no words, 0)``."""
    c = np.asarray(counts, dtype=np.int64).reshape(-1)
    end = np.cumsum(c)
    fg = ((np.arange(len(c)) & 1) == 1) & (c > 0)
    s, e = (end - c)[fg], end[fg]                                     # foreground runs [s, e) in column-major positions
    if len(s) == 0:
        return (-1, -1, -1, -1), np.zeros((0,), np.uint32), 0
    if int(e.max()) > H * W:
        raise ValueError(f"run lengths cover {int(e.max())} pixels, the frame has {H * W}")
    xs, xe = s // H, (e - 1) // H
    cross = xs < xe                                                   # (a run that goes on into the next column has rows H - 1 and 0)
    x0, x1 = int(xs.min()), int(xe.max())
    y0, y1 = int(np.where(cross, 0, s % H).min()), int(np.where(cross, H - 1, (e - 1) % H).max())
    bw = x1 - x0 + 1
    delta = np.zeros(bw * H + 1, dtype=np.int32)
    np.add.at(delta, s - x0 * H, 1)
    np.add.at(delta, e - x0 * H, -1)
    cols = (np.cumsum(delta[:-1]) > 0).reshape(bw, H).T[y0:y1 + 1]     # [rows, bw]
    c0, wc = x0 >> 5, (x1 >> 5) - (x0 >> 5) + 1
    bits = np.zeros((y1 - y0 + 1, wc * 32), dtype=bool)
    bits[:, x0 - 32 * c0: x0 - 32 * c0 + bw] = cols
    words = np.packbits(bits.reshape(-1, wc, 32), axis=-1, bitorder="little").view("<u4").reshape(-1)
    return (y0, x0, y1, x1), words.astype(np.uint32), int((e - s).sum())


def rle_crop_set(ops, runs: Sequence[Sequence[int]], H: int, W: int) -> CropMaskSet:
    """The masks given as run lengths (ground truth with ``segmentation`` as a dict) as a :class:`CropMaskSet` whose rooms are
    the tight boxes: packed on the host (:func:`rle_host_crop`), words, boxes and pixel counts uploaded in one copy."""
    M = len(runs)
    if M == 0:
        return CropMaskSet.empty(ops, (H, W))
    got = [rle_host_crop(r, H, W) for r in runs]
    room_h = np.asarray([g[0] for g in got], dtype=np.int32).reshape(M, 4)
    words = np.concatenate([g[1] for g in got] + [np.zeros((1,), np.uint32)]).view(np.int32)      # (never empty)
    tab = ops.upload(np.concatenate([room_h.reshape(-1), np.asarray([g[2] for g in got], dtype=np.int32), words]))
    return CropMaskSet(ops, (H, W), room_h, tab[5 * M:], tab[:4 * M].view(M, 4), tab[4 * M:5 * M])


def _cross(ops, D: int, G: int, det_label: Optional[np.ndarray], gt_label: Optional[np.ndarray], kernel: Callable) -> torch.Tensor:
    """What both cross matrices share: the zeroed ``[D, G]`` output, the empty cases and the uploaded table (every detection's
    first annotation and annotation count, the labels).  ``kernel(det labels, gt labels, first, count, out)`` is the one kernel
    call, on device pointers (the labels 0 when there are none)."""
    out = torch.zeros((D, max(G, 1)), dtype=torch.int32, device=ops.device)
    if D == 0 or G == 0:
        return out[:, :G]
    tab = np.concatenate([np.zeros(D, np.int32), np.full(D, G, np.int32),
                          np.asarray(det_label if det_label is not None else np.zeros(D), dtype=np.int32),
                          np.asarray(gt_label if gt_label is not None else np.zeros(G), dtype=np.int32)])
    tt = torch.from_numpy(tab).to(ops.device)
    lab = det_label is not None
    kernel(_lib.ptr(tt[2 * D:]) if lab else 0, _lib.ptr(tt[3 * D:]) if lab else 0, _lib.ptr(tt), _lib.ptr(tt[D:]), _lib.ptr(out))
    return out


def cross_matrix(ops, det: torch.Tensor, det_bbox: torch.Tensor, det_label: Optional[np.ndarray], gt: torch.Tensor,
                 gt_bbox: torch.Tensor, gt_label: Optional[np.ndarray], W: int) -> torch.Tensor:
    """``[D, G]`` int32 on the device: ``|det_i & gt_j|``, 0 where the labels differ (``demia_mask_cross_matrix``)."""
    D, H, _ = det.shape
    G = int(gt.shape[0])

    def kernel(d_lab, g_lab, first, count, out):
        _lib.check(ops.lib.demia_mask_cross_matrix(_lib.ptr(det), _lib.ptr(det_bbox), d_lab, _lib.ptr(gt), _lib.ptr(gt_bbox), g_lab, first, count,
                                                   out, D, G, H, W, ops._stream()), "demia_mask_cross_matrix")
    return _cross(ops, D, G, det_label, gt_label, kernel)


def cross_matrix_crop(ops, det: CropMaskSet, det_label: Optional[np.ndarray], gt: CropMaskSet, gt_label: Optional[np.ndarray],
                      det_bbox: Optional[torch.Tensor] = None) -> torch.Tensor:
    """:func:`cross_matrix` of two crop-framed sets over one frame (``demia_crop_cross_matrix``): the same ``[D, G]`` counts.
    ``det_bbox``: the detections' tight boxes on the device when the caller has its own copy (default: the set's)."""
    D, G = len(det), len(gt)

    def kernel(d_lab, g_lab, first, count, out):
        assert det.hw == gt.hw
        _lib.check(ops.lib.demia_crop_cross_matrix(_lib.ptr(det.payload), _lib.ptr(det.room), _lib.ptr(det.offsets),
                                                   _lib.ptr(det.bbox if det_bbox is None else det_bbox), d_lab,
                                                   _lib.ptr(gt.payload), _lib.ptr(gt.room), _lib.ptr(gt.offsets), _lib.ptr(gt.bbox),
                                                   g_lab, first, count, out, D, G, ops._stream()), "demia_crop_cross_matrix")
    return _cross(ops, D, G, det_label, gt_label, kernel)


def _plane_rle(ops, packed: torch.Tensor, bbox: torch.Tensor, W: int, n, off, counts) -> None:
    M, H, _ = packed.shape
    _lib.check(ops.lib.demia_mask_rle_colmajor(_lib.ptr(packed), _lib.ptr(bbox), _lib.ptr(n), _lib.ptr(off), _lib.ptr(counts), M, H, W,
                                               ops._stream()), "demia_mask_rle_colmajor")


def _crop_rle(ops, cset: CropMaskSet, bbox: torch.Tensor, n, off, counts) -> None:
    H, W = cset.hw
    _lib.check(ops.lib.demia_crop_rle_colmajor(_lib.ptr(cset.payload), _lib.ptr(cset.room), _lib.ptr(cset.offsets), _lib.ptr(bbox), _lib.ptr(n),
                                               _lib.ptr(off), _lib.ptr(counts), len(cset), H, W, ops._stream()), "demia_crop_rle_colmajor")


def _rle_two_pass(ops, M: int, kernel: Callable) -> Tuple[np.ndarray, np.ndarray]:
    """The encoder's two passes with a wait in between: ``kernel(n, None, None)`` counts every mask's runs, the offsets are summed
    on the host, ``kernel(None, off, counts)`` writes the runs."""
    if M == 0:
        return np.zeros((0,), np.uint32), np.zeros((1,), np.int64)
    n = torch.empty((M,), dtype=torch.int32, device=ops.device)
    kernel(n, None, None)
    off = np.zeros(M + 1, dtype=np.int64)
    np.cumsum(n.cpu().numpy(), out=off[1:])
    t_off = torch.from_numpy(off).to(ops.device)
    counts = torch.empty((int(off[-1]),), dtype=torch.int32, device=ops.device)
    kernel(None, t_off, counts)
    return counts.cpu().numpy().view(np.uint32), off


def _rle_launched(ops, M: int, room: int, kernel: Callable) -> Tuple[torch.Tensor, torch.Tensor]:
    """The encoder's two passes enqueued WITHOUT a wait in between: the offsets are summed on the device and cut at ``room``, so a
    mask whose runs do not fit leaves its slot alone (the write pass checks every slot's size)."""
    n = torch.empty((M,), dtype=torch.int32, device=ops.device)
    counts = torch.zeros((max(1, int(room)),), dtype=torch.int32, device=ops.device)
    if M == 0:
        return n, counts
    kernel(n, None, None)
    off = torch.zeros((M + 1,), dtype=torch.int64, device=ops.device)
    off[1:] = torch.cumsum(n, 0, dtype=torch.int64)
    off.clamp_(max=int(counts.shape[0]))
    kernel(None, off, counts)
    return n, counts


def rle_counts(ops, packed: torch.Tensor, bbox: torch.Tensor, W: int) -> Tuple[np.ndarray, np.ndarray]:
    """Column-major run lengths of every mask, the background run first (pycocotools' ``encode``): ``(counts uint32, offsets
    [M + 1] int64)`` on the host, mask m's runs at ``counts[offsets[m]:offsets[m + 1]]`` (``demia_mask_rle_colmajor``)."""
    return _rle_two_pass(ops, int(packed.shape[0]), partial(_plane_rle, ops, packed, bbox, W))


def rle_room(bbox: np.ndarray) -> int:
    """Room (in counts) that :func:`rle_counts_launch` reserves for masks with the HOST boxes ``bbox`` [M, 4] (y0, x0, y1, x1,
    y0 = -1 when empty): four transitions per box column and a few more per mask -- twice what a mask whose columns are single
    runs needs.  A set of masks that needs more is encoded again by :func:`rle_counts` (one more wait)."""
    bbox = np.asarray(bbox, dtype=np.int64).reshape(-1, 4)
    cols = np.where(bbox[:, 0] >= 0, bbox[:, 3] - bbox[:, 1] + 1, 0)
    return int((4 * cols + 16).sum())


def rle_counts_launch(ops, packed: torch.Tensor, bbox: torch.Tensor, W: int, room: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Both passes of ``demia_mask_rle_colmajor`` enqueued without a wait in between, into ``room`` counts.  Returns the device
    tensors ``(n_counts [M] int32, counts [room] int32)`` for the caller to fetch together with its other tables;
    :func:`rle_counts_finish` turns the host copies into ``(counts, offsets)`` or reports that the room was too small."""
    return _rle_launched(ops, int(packed.shape[0]), room, partial(_plane_rle, ops, packed, bbox, W))


def rle_counts_crop(ops, cset: CropMaskSet, bbox: Optional[torch.Tensor] = None) -> Tuple[np.ndarray, np.ndarray]:
    """:func:`rle_counts` of a crop-framed set (``demia_crop_rle_colmajor``): the same ``(counts, offsets)``, the masks read in
    their rooms.  ``bbox``: the tight boxes on the device when the caller has its own copy (default: the set's)."""
    return _rle_two_pass(ops, len(cset), partial(_crop_rle, ops, cset, cset.bbox if bbox is None else bbox))


def rle_counts_launch_crop(ops, cset: CropMaskSet, room: int, bbox: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """:func:`rle_counts_launch` of a crop-framed set: both passes enqueued without a wait, the offsets cut at ``room`` counts;
    the same ``(n_counts, counts)`` device tensors for :func:`rle_counts_finish`."""
    return _rle_launched(ops, len(cset), room, partial(_crop_rle, ops, cset, cset.bbox if bbox is None else bbox))


def rle_counts_finish(n_host: np.ndarray, counts_host: np.ndarray) -> Optional[Tuple[np.ndarray, np.ndarray]]:
    """Host side of :func:`rle_counts_launch`: ``(counts uint32, offsets [M + 1] int64)`` as :func:`rle_counts` returns them,
    or None when the runs did not fit the room."""
    off = np.zeros(len(n_host) + 1, dtype=np.int64)
    np.cumsum(n_host, dtype=np.int64, out=off[1:])
    if off[-1] > len(counts_host):
        return None
    return np.ascontiguousarray(counts_host[:off[-1]]).view(np.uint32), off


# ---- host codecs -------------------------------------------------------------------------------------------------------------
def rle_strings(counts: np.ndarray, offsets: np.ndarray) -> List[str]:
    """pycocotools' ``rleToString`` of each run list (``demia_host_rle_string``)."""
    lib = _lib.load()
    M = len(offsets) - 1
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    cap = max(1, 7 * len(counts))
    buf = C.create_string_buffer(cap)
    toff = np.zeros(M + 1, dtype=np.int64)
    got = lib.demia_host_rle_string(_ptr(counts) or 0, offsets.ctypes.data, M, buf, cap, toff.ctypes.data)
    if got < 0:
        raise RuntimeError("demia_host_rle_string: buffer too small")
    raw = buf.raw[:got].decode("ascii")
    return [raw[toff[m]:toff[m + 1]] for m in range(M)]


def rle_from_string(s: str) -> np.ndarray:
    """pycocotools' ``rleFrString``: the run lengths of a compressed RLE string."""
    cnts: List[int] = []
    p = 0
    while p < len(s):
        x = k = 0
        more = True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x & 0xffffffff)
    return np.asarray(cnts, dtype=np.int64)


def rle_decode(counts: Sequence[int], h: int, w: int) -> np.ndarray:
    """Run lengths (background first, column-major) -> (h, w) bool mask."""
    flat = np.zeros(h * w, dtype=bool)
    pos = 0
    for i, c in enumerate(counts):
        if i % 2:
            flat[pos:pos + int(c)] = True
        pos += int(c)
    return flat.reshape(w, h).T


def rle_to_bbox(counts: np.ndarray, offsets: np.ndarray, h: int) -> np.ndarray:
    """pycocotools' ``toBbox`` (``rleToBbox``, 2.0.7 on) of every run list: float64 ``[M, 4]`` XYWH.  The box is the tight box
    of the mask's pixels, EXCEPT that a foreground run that goes on into the next column (the last row of one column and the
    first row of the next are both set) makes it span all rows: y = 0, height = h.  An empty mask gives four zeros."""
    M = len(offsets) - 1
    out = np.zeros((M, 4), dtype=np.float64)
    c = np.asarray(counts, dtype=np.int64)
    if M == 0 or len(c) == 0:
        return out
    offsets = np.asarray(offsets, dtype=np.int64)
    mid = np.repeat(np.arange(M), np.diff(offsets))
    end = np.cumsum(c)
    end -= np.concatenate([[0], end])[offsets[:-1]][mid]            # the run's end within its own mask
    start = end - c
    fg = (((np.arange(len(c)) - offsets[:-1][mid]) & 1) == 1) & (c > 0)
    mid, start, last = mid[fg], start[fg], end[fg] - 1
    ys_, xs_, ye_, xe_ = start % h, start // h, last % h, last // h
    cross = xs_ < xe_
    ys_, ye_ = np.where(cross, 0, ys_), np.where(cross, h - 1, ye_)
    big = np.iinfo(np.int64).max
    xs, ys = np.full(M, big), np.full(M, big)
    xe, ye = np.full(M, -1), np.full(M, -1)
    np.minimum.at(xs, mid, xs_)
    np.minimum.at(ys, mid, ys_)
    np.maximum.at(xe, mid, xe_)
    np.maximum.at(ye, mid, ye_)
    ok = xe >= 0
    out[ok] = np.stack([xs[ok], ys[ok], xe[ok] - xs[ok] + 1, ye[ok] - ys[ok] + 1], 1)
    return out


# ---- IoU tables ---------------------------------------------------------------------------------------------------------------
def mask_iou(inter: np.ndarray, dt_area: np.ndarray, gt_area: np.ndarray, crowd: np.ndarray) -> np.ndarray:
    """``maskUtils.iou`` of RLEs from the intersection counts: ``i / u`` with ``u = |d| + |g| - i`` (``|d|`` for a crowd
    ground truth), 0 where ``i == 0``."""
    i = inter.astype(np.float64)
    u = np.where(crowd[None, :].astype(bool), dt_area[:, None].astype(np.float64),
                 dt_area[:, None].astype(np.float64) + gt_area[None, :].astype(np.float64) - i)
    return np.where(inter > 0, i / np.where(inter > 0, u, 1.0), 0.0)


BOUNDARY_RATIO = 0.02        # Boundary IoU's default dilation ratio


def boundary_width(H: int, W: int, ratio: float = BOUNDARY_RATIO, width: Optional[int] = None) -> int:
    """The erosion width ``d`` of Boundary IoU for an ``H x W`` frame (``include/deepemia_hip.h`` states the definitions):
    ``width`` itself when given (an integer >= 1), else ``max(1, int(round(ratio * sqrt(H*H + W*W))))`` with Python's ``round``."""
    if width is not None:
        if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or int(width) < 1:
            raise ValueError(f"boundary width must be an integer >= 1, got {width!r}")
        return int(width)
    return max(1, int(round(float(ratio) * float(np.sqrt(float(H) * float(H) + float(W) * float(W))))))


def boundary_iou(band_inter: np.ndarray, dt_band: np.ndarray, gt_band: np.ndarray, crowd: np.ndarray) -> np.ndarray:
    """Boundary IoU from the band counts: :func:`mask_iou` of ``|band(d) & band(g)|``, ``|band(d)|`` and ``|band(g)|`` (the
    denominator is ``|band(d)|`` for a crowd ground truth; 0 where the bands do not meet).  The band intersections are
    :func:`cross_matrix` / :func:`cross_matrix_crop` of the band sets (``MaskOps.boundary_band`` / ``CropMaskSet.boundary_band``)."""
    return mask_iou(band_inter, dt_band, gt_band, crowd)


# ---- outline agreement: surface distances per matched pair ------------------------------------------------------------------------
OUTLINE_IOU = 0.5            # a detection and an annotation are a pair from this mask IoU on
OUTLINE_TOLERANCE = 2        # NSD's tolerance in pixels: a choice, not a measurement
OUTLINE_VALUES = ("assd", "rms", "hausdorff", "hd95", "nsd", "diameter_error", "area_error")
OUTLINE_ROW_HEADER = ["image_id", "file_name", "category_id", "class_name", "detection", "annotation", "score", "iou", "detection_pixels",
                      "annotation_pixels", "detection_border", "annotation_border", "assd_px", "rms_px", "hausdorff_px", "hd95_px", "nsd",
                      "diameter_error_px", "relative_area_error"]
OUTLINE_SUMMARY_HEADER = ["class_name", "annotations", "detections", "matched", "missed", "spurious", "mean_assd_px", "median_assd_px",
                          "mean_hd95_px", "max_hausdorff_px", "mean_nsd", "mean_diameter_error_px", "mean_abs_relative_area_error"]


def outline_match(iou: np.ndarray, scores: np.ndarray, d_cat: np.ndarray, g_cat: np.ndarray, crowd: np.ndarray,
                  thr: float = OUTLINE_IOU) -> np.ndarray:
    """The pairs of the outline-agreement report for one image, ``[P, 2]`` int64 (detection, annotation) in detection order, from
    the ``segm`` IoU table (:func:`mask_iou`, f64).  Detections are taken in descending score, ties by ascending index; each
    takes the still unmatched annotation that is not a crowd region, has its category and an IoU of at least ``thr``, and among
    those the highest IoU, ties by the lower annotation index.  Crowd annotations are never matched and ``maxDets`` does not
    apply.  Deliberately not COCOeval's matcher (no ignore flags, no area ranges, one threshold): AP stays COCOeval's business."""
    iou = np.asarray(iou, dtype=np.float64).reshape(len(scores), len(g_cat))
    d_cat, g_cat = np.asarray(d_cat, dtype=np.int64), np.asarray(g_cat, dtype=np.int64)
    free = ~np.asarray(crowd).astype(bool)
    pairs = []
    for d in np.argsort(-np.asarray(scores, dtype=np.float64), kind="stable").tolist():
        ok = free & (g_cat == d_cat[d]) & (iou[d] >= thr)
        if ok.any():
            g = int(np.argmax(np.where(ok, iou[d], -1.0)))           # (argmax: the first of the highest, so the lower index)
            free[g] = False
            pairs.append((d, g))
    return np.asarray(sorted(pairs), dtype=np.int64).reshape(-1, 2)


def outline_values(rec: Dict[str, np.ndarray], d_px: np.ndarray, g_px: np.ndarray, tolerance: int = OUTLINE_TOLERANCE) -> Dict[str, np.ndarray]:
    """The report's seven values per pair, f64 from the integers alone.  ``rec``: ``OutlineAgreement.from_host``'s arrays (direction
    0: detection -> annotation, 1: the reverse); ``d_px`` / ``g_px``: the rasterised pixel counts of the pairs' two masks.
      assd            (sum_q_dg + sum_q_gd) / (256 (n_d + n_g))
      rms             sqrt((sum_d2_dg + sum_d2_gd) / (n_d + n_g))
      hausdorff       sqrt(max(max_d2_dg, max_d2_gd))
      hd95            the larger, over the two directions, of the smallest c with 100 cum_hist[c] >= 95 n; SATURATES at 127
      nsd             (cum_dg[tolerance] + cum_gd[tolerance]) / (n_d + n_g), tolerance an integer from 0 to 126
      diameter_error  2 sqrt(A_d / pi) - 2 sqrt(A_g / pi): signed, positive = the detection is too large
      area_error      (A_d - A_g) / A_g
    All lengths in pixels."""
    n = rec["n"].astype(np.int64)
    both = (n[:, 0] + n[:, 1]).astype(np.float64)
    cum = np.cumsum(rec["hist"].astype(np.int64), axis=2)
    hd95 = np.argmax(100 * cum >= 95 * n[:, :, None], axis=2).max(axis=1) if len(n) else np.zeros(0, np.int64)
    a_d, a_g = np.asarray(d_px, dtype=np.int64), np.asarray(g_px, dtype=np.int64)
    return {"assd": (rec["sum_q"][:, 0] + rec["sum_q"][:, 1]).astype(np.float64) / (256.0 * both),
            "rms": np.sqrt((rec["sum_d2"][:, 0] + rec["sum_d2"][:, 1]).astype(np.float64) / both),
            "hausdorff": np.sqrt(np.maximum(rec["max_d2"][:, 0], rec["max_d2"][:, 1]).astype(np.float64)),
            "hd95": hd95.astype(np.float64),
            "nsd": (cum[:, 0, tolerance] + cum[:, 1, tolerance]).astype(np.float64) / both,
            "diameter_error": 2.0 * np.sqrt(a_d.astype(np.float64) / np.pi) - 2.0 * np.sqrt(a_g.astype(np.float64) / np.pi),
            "area_error": (a_d - a_g).astype(np.float64) / a_g.astype(np.float64)}


class OutlineReport:
    """The outline-agreement report of one evaluate run: one row per matched pair (:func:`outline_match`, image by image) with the
    values of :func:`outline_values`, and per class the counts and the pooled statistics.  ``measure`` of :meth:`add_image` is the
    device stage: ``measure(pairs, detection pixel counts, annotation pixel counts)`` is called only for an image with a pair and
    returns ``OutlineAgreement.from_host``'s arrays."""

    def __init__(self, iou: float = OUTLINE_IOU, tolerance: int = OUTLINE_TOLERANCE):
        self.iou, self.tolerance = float(iou), int(tolerance)
        self.rows: List[list] = []
        self.counts: Dict[int, List[int]] = {}       # dataset category id -> [non-crowd annotations, detections, matched]

    def add_image(self, image_id, file_name: str, d_cat, scores, d_px, g_cat, g_px, crowd, iou: np.ndarray,
                  measure: Callable[[np.ndarray, np.ndarray, np.ndarray], Dict[str, np.ndarray]]) -> int:
        """One image: ``d_cat`` / ``g_cat`` dataset category ids, ``scores`` f64, ``d_px`` / ``g_px`` pixel counts, ``iou`` the
        ``segm`` IoU table.  Returns the number of pairs."""
        d_cat, g_cat = np.asarray(d_cat, dtype=np.int64), np.asarray(g_cat, dtype=np.int64)
        crowd = np.asarray(crowd).astype(bool)
        for c in g_cat[~crowd].tolist():
            self.counts.setdefault(c, [0, 0, 0])[0] += 1
        for c in d_cat.tolist():
            self.counts.setdefault(c, [0, 0, 0])[1] += 1
        pairs = outline_match(iou, scores, d_cat, g_cat, crowd, self.iou)
        if len(pairs) == 0:
            return 0
        d_all, g_all = np.asarray(d_px, dtype=np.int64).reshape(-1), np.asarray(g_px, dtype=np.int64).reshape(-1)
        rec = measure(pairs, d_all, g_all)
        d_px, g_px = d_all[pairs[:, 0]], g_all[pairs[:, 1]]
        val = outline_values(rec, d_px, g_px, self.tolerance)
        iou = np.asarray(iou, dtype=np.float64).reshape(len(d_cat), len(g_cat))
        for k, (d, g) in enumerate(pairs.tolist()):
            self.counts[int(d_cat[d])][2] += 1
            self.rows.append([image_id, file_name, int(d_cat[d]), d, g, float(scores[d]), float(iou[d, g]), int(d_px[k]), int(g_px[k]),
                              int(rec["n"][k, 0]), int(rec["n"][k, 1])] + [float(val[name][k]) for name in OUTLINE_VALUES])
        return len(pairs)

    def summary(self, cat_ids: Sequence[int], class_names: Sequence[str]) -> List[list]:
        """One row per class (``cat_ids`` and ``class_names`` side by side) and the row ``all``, in ``OUTLINE_SUMMARY_HEADER``'s
        columns; the values are pooled over the pairs, and None where a class has no pair."""
        out = []
        for cid, name in list(zip(cat_ids, class_names)) + [(None, "all")]:
            cnt = [sum(v[i] for k, v in self.counts.items() if cid is None or k == cid) for i in range(3)]
            rows = [r for r in self.rows if cid is None or r[2] == cid]
            v = {n: np.asarray([r[11 + i] for r in rows], dtype=np.float64) for i, n in enumerate(OUTLINE_VALUES)}
            stats = [None] * 7 if not rows else [float(v["assd"].mean()), float(np.median(v["assd"])), float(v["hd95"].mean()),
                                                 float(v["hausdorff"].max()), float(v["nsd"].mean()), float(v["diameter_error"].mean()),
                                                 float(np.abs(v["area_error"]).mean())]
            out.append([name, cnt[0], cnt[1], cnt[2], cnt[0] - cnt[2], cnt[1] - cnt[2]] + stats)
        return out

    def write(self, output_dir: str, cat_ids: Sequence[int], class_names: Sequence[str]) -> List[list]:
        """``outline_agreement.csv`` and ``outline_summary.csv`` in ``output_dir``; returns the summary rows."""
        names = dict(zip(cat_ids, class_names))
        with open(os.path.join(output_dir, "outline_agreement.csv"), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(OUTLINE_ROW_HEADER)
            for r in self.rows:
                w.writerow(r[:3] + [names.get(r[2], "")] + [repr(x) if isinstance(x, float) else x for x in r[3:]])
        summary = self.summary(cat_ids, class_names)
        with open(os.path.join(output_dir, "outline_summary.csv"), "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(OUTLINE_SUMMARY_HEADER)
            for r in summary:
                w.writerow(["" if x is None else (repr(x) if isinstance(x, float) else x) for x in r])
        return summary


# ---- error maps: one picture per image of where the detections and the ground truth differ -------------------------------------------
ERROR_MAP_IOU = 0.5          # a detection and an annotation are a pair from this mask IoU on (outline_match)
ERROR_MAP_ALPHA = 96         # weight of a fill colour, of 256
# BGR; the order is the kernel's (include/deepemia_hip.h): three fills, then the five line classes by priority
ERROR_MAP_PALETTE = ((0, 255, 0), (0, 0, 255), (255, 0, 0), (255, 0, 255), (255, 255, 0), (0, 255, 255), (255, 255, 255), (128, 128, 128))
ERROR_MAP_LABELS = ("agree (fill)", "excess: detected, not annotated (fill)", "missing: annotated, not detected (fill)",
                    "unmatched detection (line)", "missed annotation (line)", "matched detection (line)", "matched annotation (line)",
                    "crowd region (line)")
ERROR_MAP_HEADER = ["image_id", "file_name", "detections", "annotations", "matched", "missed", "spurious", "crowd", "agree_px", "excess_px",
                    "missing_px", "ignored_px", "pixel_precision", "pixel_recall", "pixel_dice"]


def error_map_line(H: int, W: int) -> int:
    """The default line width of an ``H x W`` image: ``min(4, max(1, round(max(H, W) / 1024)))``, round = Python's (half to even)."""
    return min(4, max(1, round(max(int(H), int(W)) / 1024)))


def error_map_states(pairs: np.ndarray, n_det: int, crowd: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """``(d_state [n_det], g_state [G])`` int32 for the error-map kernel from the pairs of :func:`outline_match`: a paired mask is 1,
    an unpaired one 2 (a spurious detection, a missed annotation), a crowd annotation 3."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    crowd = np.asarray(crowd).astype(bool).reshape(-1)
    d_state = np.full(int(n_det), 2, dtype=np.int32)
    g_state = np.where(crowd, 3, 2).astype(np.int32)
    d_state[pairs[:, 0]] = 1
    g_state[pairs[:, 1]] = 1
    return d_state, g_state


def error_map_ratios(agree: int, excess: int, missing: int) -> Tuple[Optional[float], Optional[float], Optional[float]]:
    """(pixel precision, pixel recall, pixel Dice) from the three integers; None where a denominator is 0."""
    def ratio(num: int, den: int) -> Optional[float]:
        return None if den == 0 else float(num) / float(den)
    return ratio(agree, agree + excess), ratio(agree, agree + missing), ratio(2 * agree, 2 * agree + excess + missing)


class ErrorMaps:
    """The error maps of one evaluate run (``--visualize``), the sibling of :class:`OutlineReport`: per test image one picture
    ``evaluation_images/<image_id>_<stem>_evaluation.png`` under ``output_dir`` and one row of ``evaluation_images.csv``.  ``paint``
    of :meth:`add_image` is the device stage: ``paint(d_state, g_state)`` returns the painted image on the host (``[H, W, 3]`` uint8
    BGR) and the four pixel counts (agree, excess, missing, ignored), from one device-to-host copy.  ``line``: the line width, or None
    for :func:`error_map_line` of each image."""

    def __init__(self, output_dir: str, iou: float = ERROR_MAP_IOU, alpha: int = ERROR_MAP_ALPHA, line: Optional[int] = None):
        self.output_dir, self.iou, self.alpha, self.line = str(output_dir), float(iou), int(alpha), (None if line is None else int(line))
        self.rows: List[list] = []

    @property
    def image_dir(self) -> str:
        return os.path.join(self.output_dir, "evaluation_images")

    def line_for(self, H: int, W: int) -> int:
        return error_map_line(H, W) if self.line is None else self.line

    def image_path(self, image_id, file_name: str) -> str:
        stem = os.path.splitext(os.path.basename(str(file_name)))[0]
        return os.path.join(self.image_dir, f"{image_id}_{stem}_evaluation.png")

    def add_image(self, image_id, file_name: str, d_cat, scores, g_cat, crowd, iou: np.ndarray,
                  paint: Callable[[np.ndarray, np.ndarray], Tuple[np.ndarray, Sequence[int]]]) -> str:
        """One image: ``d_cat`` / ``g_cat`` dataset category ids, ``scores`` f64, ``iou`` the ``segm`` IoU table.  Returns the
        picture's path."""
        from PIL import Image

        crowd = np.asarray(crowd).astype(bool).reshape(-1)
        pairs = outline_match(iou, scores, d_cat, g_cat, crowd, self.iou)
        d_state, g_state = error_map_states(pairs, len(scores), crowd)
        bgr, counts = paint(d_state, g_state)
        path = self.image_path(image_id, file_name)
        os.makedirs(self.image_dir, exist_ok=True)
        Image.fromarray(np.ascontiguousarray(np.asarray(bgr)[:, :, ::-1])).save(path)
        n_det, n_ann, n_pair = len(d_state), int((~crowd).sum()), len(pairs)
        agree, excess, missing, ignored = (int(v) for v in counts)
        self.rows.append([image_id, os.path.basename(str(file_name)), n_det, n_ann, n_pair, n_ann - n_pair, n_det - n_pair, int(crowd.sum()),
                          agree, excess, missing, ignored] + list(error_map_ratios(agree, excess, missing)))
        return path

    def write(self) -> str:
        """``evaluation_images.csv`` in ``output_dir`` and ``evaluation_images/legend.png``; returns the table's path."""
        os.makedirs(self.image_dir, exist_ok=True)
        path = os.path.join(self.output_dir, "evaluation_images.csv")
        with open(path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(ERROR_MAP_HEADER)
            for r in self.rows:
                w.writerow(["" if x is None else (repr(x) if isinstance(x, float) else x) for x in r])
        self._legend().save(os.path.join(self.image_dir, "legend.png"))
        return path

    @staticmethod
    def _legend():
        """The palette with its eight labels (Pillow's default font; no parity is claimed for it)."""
        from PIL import Image, ImageDraw

        row, pad, sw = 22, 6, 28
        im = Image.new("RGB", (360, 2 * pad + row * len(ERROR_MAP_PALETTE)), (32, 32, 32))
        d = ImageDraw.Draw(im)
        for k, ((b, g, r), label) in enumerate(zip(ERROR_MAP_PALETTE, ERROR_MAP_LABELS)):
            y = pad + k * row
            d.rectangle([pad, y + 3, pad + sw, y + row - 4], fill=(r, g, b), outline=(0, 0, 0))
            d.text((2 * pad + sw, y + 5), label, fill=(255, 255, 255))
        return im


def box_iou(dt: np.ndarray, gt: np.ndarray, crowd: np.ndarray) -> np.ndarray:
    """``maskUtils.iou``'s box branch (``bbIou``) on XYWH float64 boxes."""
    dt = np.asarray(dt, dtype=np.float64).reshape(-1, 4)
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 4)
    da = dt[:, 2] * dt[:, 3]
    ga = gt[:, 2] * gt[:, 3]
    w = np.fmin(dt[:, None, 2] + dt[:, None, 0], gt[None, :, 2] + gt[None, :, 0]) - np.fmax(dt[:, None, 0], gt[None, :, 0])
    h = np.fmin(dt[:, None, 3] + dt[:, None, 1], gt[None, :, 3] + gt[None, :, 1]) - np.fmax(dt[:, None, 1], gt[None, :, 1])
    i = w * h
    u = np.where(crowd[None, :].astype(bool), da[:, None], da[:, None] + ga[None, :] - i)
    ok = (w > 0) & (h > 0)
    return np.where(ok, i / np.where(ok, u, 1.0), 0.0)


# ---- COCOeval --------------------------------------------------------------------------------------------------------------
class EvalTables:
    """The entries of one task: per detection (image, category, score, area, its row of the task's IoU table) and per ground
    truth (image, category, area, crowd, its column).  ``add_image`` appends one image in COCOeval's list order."""

    def __init__(self):
        self.d_img, self.d_cat, self.d_score, self.d_area, self.d_row = [], [], [], [], []
        self.g_img, self.g_cat, self.g_area, self.g_crowd, self.g_col = [], [], [], [], []
        self.iou: List[np.ndarray] = []
        self._base = 0

    def add_image(self, img: int, d_cat, d_score, d_area, g_cat, g_area, g_crowd, iou: np.ndarray) -> None:
        D, G = len(d_cat), len(g_cat)
        self.d_img.append(np.full(D, img, np.int64))
        self.d_cat.append(np.asarray(d_cat, np.int64))
        self.d_score.append(np.asarray(d_score, np.float64))
        self.d_area.append(np.asarray(d_area, np.float64))
        self.d_row.append(self._base + np.arange(D, dtype=np.int64) * G)
        self.g_img.append(np.full(G, img, np.int64))
        self.g_cat.append(np.asarray(g_cat, np.int64))
        self.g_area.append(np.asarray(g_area, np.float64))
        self.g_crowd.append(np.asarray(g_crowd, np.uint8))
        self.g_col.append(np.arange(G, dtype=np.int64))
        flat = np.ascontiguousarray(iou, dtype=np.float64).reshape(-1)
        assert flat.size == D * G
        self.iou.append(flat)
        self._base += D * G

    def cat(self, name):
        v = getattr(self, name)
        return np.concatenate(v) if v else np.zeros((0,))


def check_max_dets(max_dets: Optional[Sequence[int]]) -> List[int]:
    """``params.maxDets``: three ascending positive counts (default ``MAX_DETS``); the last is the one AP / AR use."""
    md = list(MAX_DETS) if max_dets is None else [int(v) for v in max_dets]
    if len(md) != 3 or md[0] < 1 or any(b <= a for a, b in zip(md, md[1:])):
        raise ValueError(f"max_dets must be three ascending positive counts, got {max_dets!r}")
    return md


def evaluate(tables: Dict[str, EvalTables], img_ids: Sequence[int], cat_ids: Sequence[int],
             max_dets: Optional[Sequence[int]] = None) -> Dict[str, dict]:
    """``COCOeval.evaluate()`` + ``accumulate()`` for every task of ``tables`` with one native matching call:
    ``{task: {"precision": [T, R, K, A, M], "recall": [T, K, A, M], "stats": [12]}}``; ``img_ids`` / ``cat_ids`` as
    ``params.imgIds`` / ``params.catIds`` (sorted), ``max_dets`` as ``params.maxDets`` (default ``[1, 10, 100]``)."""
    max_dets = check_max_dets(max_dets)
    img_ids = np.asarray(sorted(img_ids), dtype=np.int64)
    cat_ids = np.asarray(sorted(cat_ids), dtype=np.int64)
    tasks = list(tables)
    # one group per (task, category, image) with a detection or a ground truth; groups in (task, category, image) order,
    # entries inside a group in the image's list order
    d_parts, g_parts, ious = [], [], []
    base = 0
    for ti, task in enumerate(tasks):
        t = tables[task]
        dc = t.cat("d_cat").astype(np.int64)
        gc = t.cat("g_cat").astype(np.int64)
        d_parts.append(dict(task=np.full(len(dc), ti), cat=dc, img=t.cat("d_img").astype(np.int64), score=t.cat("d_score"),
                            area=t.cat("d_area"), row=t.cat("d_row").astype(np.int64) + base))
        g_parts.append(dict(task=np.full(len(gc), ti), cat=gc, img=t.cat("g_img").astype(np.int64), area=t.cat("g_area"),
                            crowd=t.cat("g_crowd").astype(np.uint8), col=t.cat("g_col").astype(np.int64)))
        iou = t.cat("iou").astype(np.float64)
        ious.append(iou)
        base += len(iou)
    d = {k: np.concatenate([p[k] for p in d_parts]) for k in d_parts[0]} if d_parts else {}
    g = {k: np.concatenate([p[k] for p in g_parts]) for k in g_parts[0]} if g_parts else {}
    iou = np.ascontiguousarray(np.concatenate(ious) if ious else np.zeros((1,)))
    nI, nK = len(img_ids), len(cat_ids)
    img_pos = {int(v): i for i, v in enumerate(img_ids)}
    cat_pos = {int(v): i for i, v in enumerate(cat_ids)}
    # keep only entries of listed images / categories (COCOeval's _prepare selects by params)
    def key_of(part):
        ip = np.array([img_pos.get(int(v), -1) for v in part["img"]], dtype=np.int64)
        kp = np.array([cat_pos.get(int(v), -1) for v in part["cat"]], dtype=np.int64)
        ok = (ip >= 0) & (kp >= 0)
        return (part["task"] * nK + kp) * nI + ip, ok
    dkey, dok = key_of(d)
    gkey, gok = key_of(g)
    dsel = np.nonzero(dok)[0][np.argsort(dkey[dok], kind="mergesort")]
    gsel = np.nonzero(gok)[0][np.argsort(gkey[gok], kind="mergesort")]
    dkey, gkey = dkey[dsel], gkey[gsel]
    groups = np.union1d(dkey, gkey)
    Gn = len(groups)
    dt_off = np.searchsorted(dkey, np.append(groups, np.iinfo(np.int64).max), side="left").astype(np.int64)
    dt_off[-1] = len(dkey)
    gt_off = np.searchsorted(gkey, np.append(groups, np.iinfo(np.int64).max), side="left").astype(np.int64)
    gt_off[-1] = len(gkey)
    ds = {k: np.ascontiguousarray(v[dsel]) for k, v in d.items()}
    gs = {k: np.ascontiguousarray(v[gsel]) for k, v in g.items()}
    ndt, ngt = len(dsel), len(gsel)
    A, T = len(AREA_RNG), len(IOU_THRS)
    rank = np.full(ndt, -1, dtype=np.int32)
    matched = np.zeros((A, T, ndt), dtype=np.uint8)
    dig = np.zeros((A, T, ndt), dtype=np.uint8)
    gig = np.zeros((A, ngt), dtype=np.uint8)
    score = ds["score"].astype(np.float64)
    darea = ds["area"].astype(np.float64)
    drow = ds["row"].astype(np.int64)
    garea = gs["area"].astype(np.float64)
    gcrowd = gs["crowd"].astype(np.uint8)
    gcol = gs["col"].astype(np.int64)
    rng = np.ascontiguousarray(AREA_RNG)
    thr = np.ascontiguousarray(IOU_THRS)
    _lib.check(_lib.load().demia_host_coco_match(Gn, dt_off.ctypes.data, gt_off.ctypes.data, _ptr(score), _ptr(darea), _ptr(drow),
                                                 _ptr(garea), _ptr(gcrowd), _ptr(gcol), iou.ctypes.data, rng.ctypes.data, A,
                                                 thr.ctypes.data, T, max_dets[-1], _ptr(rank), _ptr(matched), _ptr(dig), _ptr(gig)),
               "demia_host_coco_match")
    out = {}
    R, M = len(REC_THRS), len(max_dets)
    dgrp = np.searchsorted(groups, dkey) if ndt else np.zeros(0, np.int64)
    ggrp = np.searchsorted(groups, gkey) if ngt else np.zeros(0, np.int64)
    for ti, task in enumerate(tasks):
        precision = -np.ones((T, R, nK, A, M))
        recall = -np.ones((T, nK, A, M))
        for k in range(nK):
            lo_key, hi_key = (ti * nK + k) * nI, (ti * nK + k + 1) * nI
            dsl = slice(np.searchsorted(dkey, lo_key), np.searchsorted(dkey, hi_key))
            gsl = slice(np.searchsorted(gkey, lo_key), np.searchsorted(gkey, hi_key))
            if dsl.stop - dsl.start == 0 and gsl.stop - gsl.start == 0:
                continue
            # the detections of this category in COCOeval's concatenation order: image by image, by rank
            dr = rank[dsl]
            order = np.lexsort((dr, dgrp[dsl]))
            for a in range(A):
                npig = int(np.count_nonzero(gig[a, gsl] == 0))
                if npig == 0:
                    continue
                for mi, maxDet in enumerate(max_dets):
                    keep = order[(dr[order] >= 0) & (dr[order] < maxDet)]
                    sc = score[dsl][keep]
                    inds = np.argsort(-sc, kind="mergesort")
                    dtm = matched[a][:, dsl][:, keep][:, inds].astype(bool)
                    dti = dig[a][:, dsl][:, keep][:, inds].astype(bool)
                    tps = np.logical_and(dtm, np.logical_not(dti))
                    fps = np.logical_and(np.logical_not(dtm), np.logical_not(dti))
                    tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                    fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        nd = len(tp)
                        rc = tp / npig
                        pr = tp / (fp + tp + np.spacing(1))
                        recall[t, k, a, mi] = rc[-1] if nd else 0
                        pr = np.maximum.accumulate(pr[::-1])[::-1] if nd else pr
                        q = np.zeros((R,))
                        idx = np.searchsorted(rc, REC_THRS, side="left")
                        ok = idx < nd
                        q[ok] = pr[idx[ok]]            # recall points past the last detection stay 0
                        precision[t, :, k, a, mi] = q
        out[task] = {"precision": precision, "recall": recall, "stats": summarize(precision, recall, max_dets)}
    return out


def _summ(precision, recall, ap=1, iou_thr=None, area="all", mind=2) -> float:
    aind = [i for i, lbl in enumerate(AREA_LBL) if lbl == area]
    mind = [mind]
    if ap == 1:
        s = precision
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, aind, mind]
    else:
        s = recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, aind, mind]
    return -1.0 if len(s[s > -1]) == 0 else float(np.mean(s[s > -1]))


# (AP / AR, IoU threshold, area label, index into max_dets) of COCOeval.summarize()'s twelve numbers (``_summarizeDets``)
_SPEC = [(1, None, "all", 2), (1, .5, "all", 2), (1, .75, "all", 2), (1, None, "small", 2), (1, None, "medium", 2),
         (1, None, "large", 2), (0, None, "all", 0), (0, None, "all", 1), (0, None, "all", 2), (0, None, "small", 2),
         (0, None, "medium", 2), (0, None, "large", 2)]


def summarize(precision: np.ndarray, recall: np.ndarray, max_dets: Optional[Sequence[int]] = None) -> np.ndarray:
    """``COCOeval.summarize()``'s twelve numbers (``_summarizeDets``); every AP and the area ARs at the last of ``max_dets``
    (pycocotools reads its first AP at a literal 100, which is the last entry of its default)."""
    check_max_dets(max_dets)
    return np.array([_summ(precision, recall, ap, thr, area, mi) for ap, thr, area, mi in _SPEC])


def summary_lines(stats: np.ndarray, max_dets: Optional[Sequence[int]] = None) -> List[str]:
    """The twelve lines ``COCOeval.summarize()`` prints."""
    md = check_max_dets(max_dets)
    lines = []
    for (ap, thr, area, mi), v in zip(_SPEC, stats):
        title = "Average Precision" if ap == 1 else "Average Recall"
        typ = "(AP)" if ap == 1 else "(AR)"
        iou = "{:0.2f}:{:0.2f}".format(IOU_THRS[0], IOU_THRS[-1]) if thr is None else "{:0.2f}".format(thr)
        lines.append(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(title, typ, iou, area, md[mi], v))
    return lines


def derive_results(stats: np.ndarray, precision: np.ndarray, class_names: Sequence[str]) -> Dict[str, float]:
    """Detectron2's ``COCOEvaluator._derive_coco_results``: AP, AP50, AP75, APs, APm, APl and ``AP-<class>``, x100, nan where
    COCO reports -1."""
    res = {m: float(stats[i] * 100 if stats[i] >= 0 else "nan") for i, m in enumerate(METRICS)}
    assert len(class_names) == precision.shape[2]
    for k, name in enumerate(class_names):
        p = precision[:, :, k, 0, -1]
        p = p[p > -1]
        ap = np.mean(p) if p.size else float("nan")
        res[f"AP-{name}"] = float(ap * 100)
    return res
