"""The case table of the boundary-band tests: the smallest frames, masks and widths at which the band kernel can go wrong.

Frames: the smallest; the word boundary at 31 / 32 / 33 and 64 / 65 columns; a width that is no multiple of 32; and 640 x 640,
where the box region of a frame-sized mask (640 rows x 20 words) exceeds the 8192-word LDS buffer and works in global scratch.
Widths: around 1, around the word size, the default of a 2048^2 frame (58), and one larger than the frame; the 640^2 frame
runs d = 1 and d = 58 only."""
import functools

import numpy as np

FRAMES = [(1, 1), (5, 31), (5, 32), (5, 33), (40, 64), (40, 65), (70, 100), (640, 640)]
WIDTHS = (1, 2, 3, 31, 32, 33, 58)
LARGE_WORDS = 8192


def widths(H, W):
    if (H, W) == (640, 640):
        return (1, 58)
    return WIDTHS + (max(H, W) + 5,)


def _blob(rng, H, W):
    """A union of up to three ellipses anywhere in the frame (clipped by it), radii from 1 px to half the frame; every third blob
    loses 3 % of its pixels, which leaves pinholes that an erosion widens."""
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.zeros((H, W), dtype=bool)
    for _ in range(rng.randint(1, 4)):
        cy, cx = rng.uniform(0, H), rng.uniform(0, W)
        ry, rx = rng.uniform(1, max(1.5, H / 2)), rng.uniform(1, max(1.5, W / 2))
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
    if rng.randint(3) == 0:
        m &= rng.rand(H, W) >= .03
    return m


@functools.lru_cache(maxsize=None)
def masks(H, W, d):
    """(names, dense [M, H, W] bool) for frame H x W at width d.  Everything is clipped to the frame."""
    rng = np.random.RandomState(1000 * H + W)          # (the blobs do not depend on d)
    names, out = [], []

    def add(name, m):
        names.append(name)
        out.append(m)

    def rect(y0, x0, y1, x1):                          # inclusive, clipped
        m = np.zeros((H, W), dtype=bool)
        m[max(y0, 0):max(y1 + 1, 0), max(x0, 0):max(x1 + 1, 0)] = True
        return m

    add("pixel", rect(H // 2, W // 2, H // 2, W // 2))
    add("pixel_first", rect(0, 0, 0, 0))
    add("pixel_last", rect(H - 1, W - 1, H - 1, W - 1))
    add("empty", np.zeros((H, W), dtype=bool))
    add("full", np.ones((H, W), dtype=bool))
    h, w = H // 3 + 1, W // 3 + 1
    add("edge_top", rect(0, W // 3, h - 1, W // 3 + w - 1))
    add("edge_bottom", rect(H - h, W // 3, H - 1, W // 3 + w - 1))
    add("edge_left", rect(H // 3, 0, H // 3 + h - 1, w - 1))
    add("edge_right", rect(H // 3, W - w, H // 3 + h - 1, W - 1))
    add("corner_tl", rect(0, 0, h - 1, w - 1))
    add("corner_tr", rect(0, W - w, h - 1, W - 1))
    add("corner_bl", rect(H - h, 0, H - 1, w - 1))
    add("corner_br", rect(H - h, W - w, H - 1, W - 1))
    for k in (2 * d, 2 * d + 1, 2 * d + 2):            # squares around the side at which an eroded pixel first survives,
        x0 = max(0, 32 - (k + 1) // 2)                 # across the bit-31 / 32 boundary where the frame is wide enough
        add(f"square_{k}", rect(1, x0, k, x0 + k - 1))
        add(f"square_{k}_at_0", rect(0, 0, k - 1, k - 1))
    ring = rect(1, 1, H - 2, W - 2) & ~rect(H // 2 - H // 8, W // 2 - W // 8, H // 2 + H // 8, W // 2 + W // 8)
    add("square_with_hole", ring)
    add("line_h", rect(H // 2, 0, H // 2, W - 1))
    add("line_v", rect(0, min(W - 1, 32), H - 1, min(W - 1, 32)))
    for i in range(64):
        add(f"blob_{i}", _blob(rng, H, W))
    return tuple(names), np.stack(out)


def grown_rooms(rng, boxes, H, W, grow=9):
    """Rooms around the tight boxes ``[M, 4]`` (y0, x0, y1, x1; -1 = empty), grown by up to ``grow`` pixels on every side."""
    room = np.array(boxes, dtype=np.int32).reshape(-1, 4)
    ok = room[:, 0] >= 0
    g = rng.randint(0, grow + 1, room.shape)
    room[:, 0] = np.maximum(0, room[:, 0] - g[:, 0])
    room[:, 1] = np.maximum(0, room[:, 1] - g[:, 1])
    room[:, 2] = np.minimum(H - 1, room[:, 2] + g[:, 2])
    room[:, 3] = np.minimum(W - 1, room[:, 3] + g[:, 3])
    room[~ok] = -1
    return room
