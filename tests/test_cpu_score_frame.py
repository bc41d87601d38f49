"""CPU tests of the evaluate task's one scorer (``functions.evaluate_model._score``) against a stand-in frame: ``_DenseFrame``
implements the score frame's methods over boolean NumPy masks and CPU tensors -- intersections by ``&``, bands by a literal
erosion, column-major run lengths by a flat scan, outline records from ``outline_ref`` -- so the host side of the scorer (the
one copy and its layout, the result rows, the three IoU tables, the outline report's rows) runs without a GPU and is compared,
exactly, with ``coco_ref``, ``boundary_ref``, ``outline_ref`` and direct NumPy arithmetic."""
import itertools
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import boundary_ref as BR  # noqa: E402
import coco_ref as R  # noqa: E402
import coco_ref_ext as X  # noqa: E402
import outline_ref as OR  # noqa: E402

H, W = 40, 70                               # three word columns, the last one partial
IDS = {0: 7, 1: 9}                          # contiguous class -> dataset category id
WIDTH = 2                                   # evaluation.boundary_width
IOU, TOLERANCE = 0.5, 2
_BANDS = {}


def _band(m, d):
    key = (m.tobytes(), d)
    if key not in _BANDS:
        _BANDS[key] = m & ~BR.eroded_literal(m, d)
    return _BANDS[key]


def _runs(m):
    """Column-major run lengths of one mask, the background run first."""
    flat = m.T.reshape(-1)
    out, prev, c = [], False, 0
    for b in flat.tolist():
        if b != prev:
            out.append(c)
            prev, c = b, 0
        c += 1
    return out + [c]


class _DenseFrame:
    """The score frame over dense masks: ``det`` [n, H, W] and ``gt`` [G, H, W] bool.  ``err``: the error word that
    ``ground_truth`` hands back (None: none); ``short``: how many counts the run-length room falls short of what the masks need."""

    def __init__(self, det, gt, err=None, short=0):
        self.hw, self.det, self.gt, self.err, self.short = det.shape[1:], det, gt, err, short
        self.again = 0

    def ground_truth(self, anns):
        assert len(anns) == len(self.gt)
        self.gt_area = torch.from_numpy(self.gt.sum(axis=(1, 2)).astype(np.int32))
        return [] if self.err is None else [torch.tensor([self.err], dtype=torch.int32)]

    @staticmethod
    def _cross(a, b, la, lb):
        inter = (a[:, None] & b[None]).sum(axis=(2, 3)) * (np.asarray(la)[:, None] == np.asarray(lb)[None, :])
        return torch.from_numpy(inter.astype(np.int32).reshape(len(a), len(b)))

    def cross(self, det_labels, gt_labels):
        return self._cross(self.det, self.gt, det_labels, gt_labels)

    def bands(self, d, det_labels, gt_labels):
        db = np.stack([_band(m, d) for m in self.det]) if len(self.det) else self.det
        gb = np.stack([_band(m, d) for m in self.gt]) if len(self.gt) else self.gt
        return (self._cross(db, gb, det_labels, gt_labels), torch.from_numpy(db.sum(axis=(1, 2)).astype(np.int32)),
                torch.from_numpy(gb.sum(axis=(1, 2)).astype(np.int32)))

    def rle_launch(self, room):
        runs = [_runs(m) for m in self.det]
        total = sum(len(r) for r in runs)
        assert room >= total                                         # (what the scorer reserves is enough for these masks)
        counts, at = np.zeros(max(1, total - self.short), dtype=np.int32), 0
        for r in runs:                                               # a mask whose runs do not fit leaves its slot alone
            if at + len(r) <= len(counts):
                counts[at:at + len(r)] = r
            at += len(r)
        return torch.tensor([len(r) for r in runs], dtype=torch.int32), torch.from_numpy(counts)

    def rle_again(self):
        self.again += 1
        runs = [_runs(m) for m in self.det]
        off = np.zeros(len(runs) + 1, dtype=np.int64)
        np.cumsum([len(r) for r in runs], out=off[1:])
        return np.asarray([c for r in runs for c in r], dtype=np.uint32), off

    def outline(self, pairs, d_px, g_px):
        rec = OR.records(self.det, self.gt, pairs)
        head = np.stack([rec[k] for k in ("n", "max_d2", "sum_d2", "sum_q")], axis=2).astype(np.int64)            # [P, 2, 4]
        words = np.concatenate([np.ascontiguousarray(head).view(np.int32).reshape(len(head), 2, 8), rec["hist"].astype(np.int32)], axis=2)
        return SimpleNamespace(records=torch.from_numpy(np.ascontiguousarray(words)))


def _scene():
    rng = np.random.RandomState(5)
    det = np.zeros((3, H, W), dtype=bool)
    det[0, 5:20, 10:40] = True                                       # (crosses the first word boundary)
    det[2, 22:38, 28:69] = rng.rand(16, 41) < .9                     # det[1] stays empty
    gt = np.zeros((3, H, W), dtype=bool)
    gt[0, 6:22, 12:42] = True
    gt[1, 18:40, 20:70] = rng.rand(22, 50) < .5                      # the crowd region
    gt[2, 23:39, 30:70] = True                                       # (up to the last column)
    classes, scores = np.asarray([0, 1, 1], dtype=np.int64), np.asarray([0.9, 0.8, 0.7], dtype=np.float64)
    anns = [{"category_id": 0, "iscrowd": 0, "area": 450.5, "bbox": [12.0, 6.0, 42.0, 22.0], "bbox_mode": "XYXY_ABS", "segmentation": []},
            {"category_id": 1, "iscrowd": 1, "area": float(gt[1].sum()), "bbox": [20.0, 18.0, 50.0, 22.0], "bbox_mode": "XYWH_ABS", "segmentation": []},
            {"category_id": 1, "iscrowd": 0, "area": 640.0, "bbox": [30.0, 23.0, 40.0, 16.0], "bbox_mode": "XYWH_ABS", "segmentation": []}]
    return det, gt, classes, scores, anns


def _det(det, classes, scores):
    boxes = np.asarray([BR.tight_box(m) for m in det], dtype=np.int32).reshape(-1, 4)
    return classes, scores, det.sum(axis=(1, 2)).astype(np.int64), boxes


def _bb_iou(d, g, crowd):
    w = min(d[2] + d[0], g[2] + g[0]) - max(d[0], g[0])
    h = min(d[3] + d[1], g[3] + g[1]) - max(d[1], g[1])
    if not (w > 0 and h > 0):
        return 0.0
    return w * h / (d[2] * d[3] if crowd else d[2] * d[3] + g[2] * g[3] - w * h)


def _want(det, gt, classes, scores, anns, boxes=None):
    """The result rows, the three IoU tables (row-major) and the report's rows from the references."""
    n, G = len(det), len(gt)
    crowd = [a["iscrowd"] for a in anns]
    runs = [R.encode(m) for m in det]
    boxes = [X.to_bbox(r, H, W) for r in runs] if boxes is None else boxes
    rows = [{"image_id": 3, "category_id": int(classes[k]), "bbox": [float(v) for v in boxes[k]], "score": float(scores[k]),
             "segmentation": {"size": [H, W], "counts": R.to_string(runs[k])}} for k in range(n)]
    g_box = [a["bbox"] if a["bbox_mode"] == "XYWH_ABS" else [a["bbox"][0], a["bbox"][1], a["bbox"][2] - a["bbox"][0], a["bbox"][3] - a["bbox"][1]]
             for a in anns]
    same = [[classes[d] == anns[g]["category_id"] for g in range(G)] for d in range(n)]
    segm = np.asarray([[BR.mask_iou(det[d], gt[g], crowd[g]) if same[d][g] else 0.0 for g in range(G)] for d in range(n)]).reshape(n, G)
    bnd = np.asarray([[min(segm[d, g], BR.boundary_iou(det[d], gt[g], WIDTH, crowd[g])) if same[d][g] else 0.0 for g in range(G)]
                      for d in range(n)]).reshape(n, G)
    bbox = np.asarray([[_bb_iou(boxes[d], g_box[g], crowd[g]) for g in range(G)] for d in range(n)]).reshape(n, G)
    d_px, g_px = [int(m.sum()) for m in det], [int(m.sum()) for m in gt]
    d_cat, g_cat = [IDS[int(c)] for c in classes], [IDS[a["category_id"]] for a in anns]
    report = []
    for d, g in OR.match(segm, scores, d_cat, g_cat, crowd, IOU):
        dg, gd = OR.directed(det[d], gt[g]), OR.directed(gt[g], det[d])
        v = OR.values(dg, gd, d_px[d], g_px[g], TOLERANCE)
        report.append([3, "img.png", d_cat[d], d, g, float(scores[d]), segm[d, g], d_px[d], g_px[g], dg["n"], gd["n"]]
                      + [v[k] for k in ("assd", "rms", "hausdorff", "hd95", "nsd", "diameter_error", "area_error")])
    return rows, {"segm": segm, "boundary": bnd, "bbox": bbox}, report


def _run(frame, classes, scores, anns, boundary, report, boxes=None):
    from deepemia_amd import cocoeval as CE
    from deepemia_amd.functions.evaluate_model import _new_tables, _score

    rec = {"file_name": "dir/img.png", "image_id": 3, "height": H, "width": W, "annotations": anns}
    tables = _new_tables((0.02, WIDTH) if boundary else None)
    rep = CE.OutlineReport(IOU, TOLERANCE) if report else None
    copies, cpu = [0], torch.Tensor.cpu

    def spy(self, *a, **k):
        copies[0] += 1
        return cpu(self, *a, **k)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", spy)
        rows = _score(frame, rec, _det(frame.det, classes, scores), tables, IDS, (0.02, WIDTH) if boundary else None, rep, boxes_xywh=boxes)
    return rows, tables, rep, copies[0]


def _check(got, want, n, G):
    rows, tables, rep, _ = got
    w_rows, w_iou, w_report = want
    assert rows == {"instances": w_rows}
    for task, t in tables.items():
        assert np.array_equal(t.cat("iou").reshape(n, G), w_iou[task]), task
    if rep is not None:
        assert rep.rows == w_report


@pytest.mark.parametrize("boundary,report,err", list(itertools.product([False, True], [False, True], [None, 0])))
def test_scorer_on_a_dense_frame_equals_the_references(boundary, report, err):
    det, gt, classes, scores, anns = _scene()
    want = _want(det, gt, classes, scores, anns)
    assert (want[1]["segm"] > 0).sum() == 3 and len(want[2]) == 2 and want[1]["segm"][2, 1] > 0            # two pairs; the crowd column is met
    assert (want[1]["boundary"] < want[1]["segm"]).any() and want[0][1]["bbox"] == [0.0] * 4
    got = _run(_DenseFrame(det, gt, err=err), classes, scores, anns, boundary, report)
    _check(got, want, 3, 3)
    assert list(got[1]) == ["bbox", "segm"] + (["boundary"] if boundary else [])
    assert got[3] == (2 if report else 1)                            # the one copy, and one more for an image with pairs
    t = got[1]["segm"]
    assert t.cat("d_cat").tolist() == [7, 9, 9] and t.cat("g_cat").tolist() == [7, 9, 9] and t.cat("g_crowd").tolist() == [0, 1, 0]
    assert t.cat("d_area").tolist() == [float(m.sum()) for m in det] and t.cat("g_area").tolist() == [450.5, float(gt[1].sum()), 640.0]
    if report:
        assert got[2].counts == {7: [1, 1, 1], 9: [1, 2, 1]}


def test_regressed_boxes_replace_the_run_lengths_boxes():
    det, gt, classes, scores, anns = _scene()
    boxes = np.asarray([[9.5, 4.25, 31.0, 16.5], [1.0, 2.0, 3.0, 4.0], [27.0, 21.5, 42.5, 17.0]], dtype=np.float64)
    got = _run(_DenseFrame(det, gt), classes, scores, anns, True, True, boxes=boxes)
    _check(got, _want(det, gt, classes, scores, anns, boxes=boxes.tolist()), 3, 3)


def test_no_pair_costs_no_copy_and_an_error_word_raises():
    from deepemia_amd import _lib

    det, gt, classes, scores, anns = _scene()
    got = _run(_DenseFrame(det, gt[:, ::-1, ::-1].copy()), classes, scores, anns, False, True)          # (flipped: nothing reaches 0.5)
    assert got[3] == 1 and got[2].rows == []
    for word, text in ((1, "overflowed"), (2, "outside its mask's room")):
        with pytest.raises(_lib.HipKernelError, match=text):
            _run(_DenseFrame(det, gt, err=word), classes, scores, anns, False, False)


@pytest.mark.parametrize("boundary,report", [(False, False), (True, True)])
def test_no_detection_and_no_annotation(boundary, report):
    det, gt, classes, scores, anns = _scene()
    for n, G in ((0, 3), (3, 0), (0, 0)):
        d, g, c, s, a = det[:n], gt[:G], classes[:n], scores[:n], anns[:G]
        got = _run(_DenseFrame(d, g, err=0), c, s, a, boundary, report)
        _check(got, _want(d, g, c, s, a), n, G)
        assert got[3] == 1 and len(got[0]["instances"]) == n
        assert got[1]["segm"].cat("g_cat").tolist() == [7, 9, 9][:G]


def test_a_room_one_count_short_encodes_again_once_and_gives_the_same_rows():
    det, gt, classes, scores, anns = _scene()
    want = _want(det, gt, classes, scores, anns)
    full, short = _DenseFrame(det, gt), _DenseFrame(det, gt, short=1)
    _check(_run(full, classes, scores, anns, True, True), want, 3, 3)
    got = _run(short, classes, scores, anns, True, True)
    _check(got, want, 3, 3)
    assert (full.again, short.again) == (0, 1) and got[3] == 2
