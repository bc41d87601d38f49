"""The case table of the outline-agreement suites (``test_cpu_outline.py``, ``test_gpu_outline.py``): the smallest dense masks
that can break the border stage, the distance kernel's work split and its integer outputs.  A case is ``(name, det [D, H, W]
bool, gt [G, H, W] bool, pairs [P, 2])``."""
import numpy as np

TILE, SHARE = 2048, 1024          # the library's sizes when nobody asks it (demia_outline_target_tile / _source_share)


def _disc(H, W, cy, cx, r_out, r_in=-1.0):
    y, x = np.mgrid[:H, :W]
    d = (y - cy) ** 2 + (x - cx) ** 2
    return (d <= r_out * r_out) & (d > r_in * r_in if r_in >= 0 else True)


def _frame_case():
    """45 x 70 (W no multiple of 32): rectangles across the 32-pixel word boundary, a mask on all four frame edges, identical
    masks, one-pixel masks coincident and apart, a ring against a disc; some masks in two pairs, some in none."""
    H, W = 45, 70
    det, gt = np.zeros((7, H, W), bool), np.zeros((7, H, W), bool)
    det[0, 5:21, 28:41] = True
    gt[0, 7:23, 30:46] = True
    det[1] = True                                     # the whole frame: its border is the frame's edge
    gt[1, 1:H - 1, 0:W] = True                        # ... against a mask on two edges only
    rng = np.random.RandomState(4)
    blob = np.zeros((H, W), bool)
    blob[12:30, 20:50] = rng.rand(18, 30) < .8
    det[2], gt[2] = blob, blob                        # identical: everything 0
    det[3, 10, 10] = gt[3, 10, 10] = True             # one pixel, coincident
    det[4, 3, 3] = True
    gt[4, 40, 66] = True                              # one pixel each, apart
    det[5] = _disc(H, W, 22, 35, 15, 10)              # a ring ...
    gt[5] = _disc(H, W, 22, 35, 12)                   # ... against a disc: the directed distances differ
    det[6, 30:40, 60:70] = True                       # never named
    gt[6, 0:4, 0:33] = True                           # never named
    pairs = [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4), (5, 5), (0, 2), (2, 0), (5, 1), (1, 5)]
    return "frame_45x70", det, gt, np.asarray(pairs)


def _bins_case():
    """One-pixel masks at chosen offsets: d2 = 126^2, 126^2 + 1 and 127^2 (the saturating bin and its neighbours), d2 = 2 and
    perfect squares (q's floor), d2 = 0."""
    H, W = 130, 131
    offs = [(0, 126), (1, 126), (0, 127), (1, 1), (0, 3), (3, 4), (0, 0), (0, 1), (2, 3), (89, 90), (129, 130)]
    det = np.zeros((1, H, W), bool)
    det[0, 0, 0] = True
    gt = np.zeros((len(offs), H, W), bool)
    for i, (y, x) in enumerate(offs):
        gt[i, y, x] = True
    return "bins", det, gt, np.asarray([(0, i) for i in range(len(offs))])


def _far_case():
    """A 1 x 47000 frame with two far points: d2 = 46999^2 > 2^31."""
    det, gt = np.zeros((1, 1, 47000), bool), np.zeros((1, 1, 47000), bool)
    det[0, 0, 0] = True
    gt[0, 0, 46999] = True
    return "far_1x47000", det, gt, np.asarray([(0, 0)])


def _checker_case(tile, share):
    """Checkerboard blocks, where every pixel is a border pixel: more target points than twice the LDS tile and not a multiple of
    it, more source points than two workgroups' share -- in both directions; a small mask against them as well."""
    need = max(2 * tile, 2 * share) + 1
    cols = 90
    rows = -(-2 * (need + 150) // cols)
    while ((rows * cols + 1) // 2) % tile == 0 or ((rows * cols) // 2) % tile == 0:
        rows += 1
    H, W = rows + 9, cols + 40
    y, x = np.mgrid[:H, :W]
    board = (y + x) % 2 == 0
    det, gt = np.zeros((2, H, W), bool), np.zeros((2, H, W), bool)
    det[0, 2:2 + rows, 3:3 + cols] = board[2:2 + rows, 3:3 + cols]
    gt[0, 6:6 + rows, 30:30 + cols] = ~board[6:6 + rows, 30:30 + cols]
    det[1, 4:9, 100:118] = True
    gt[1, 0:3, 0:40] = True
    for m in (det[0], gt[0]):
        n = int(m.sum())
        assert n > 2 * tile and n % tile != 0 and n > 2 * share
    return "checkerboard", det, gt, np.asarray([(0, 0), (1, 0), (0, 1)])


def cases(tile: int = TILE, share: int = SHARE):
    return [_frame_case(), _bins_case(), _far_case(), _checker_case(tile, share)]


def edge_lists():
    """Pair-list edge sizes on the 45 x 70 case: ``P = 0`` with masks on both sides, and an empty side (``M = 0``)."""
    _, det, gt, _ = _frame_case()
    none = np.zeros((0, 2), dtype=np.int64)
    return [("no_pairs", det, gt, none), ("no_detections", det[:0], gt, none), ("no_annotations", det, gt[:0], none),
            ("nothing", det[:0], gt[:0], none)]
