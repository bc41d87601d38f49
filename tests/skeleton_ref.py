"""A literal reference of ``demia_mask_skeleton`` / ``demia_crop_skeleton`` (definition: ``include/deepemia_hip.h``), sharing no
code and no bit trick with the kernel: the mask is a byte per pixel with one zero ring around it, a sub-iteration is a scalar loop
that reads a pixel's eight neighbours by the names of the definition (p2 = N, p3 = NE, ... p9 = NW, y downwards) and evaluates
``C``, ``N1``, ``N2`` and ``m`` as written there; the six counts per contour are scalar loops over the skeleton pixels of the
component, which ``scipy.ndimage.label`` finds with the 3 x 3 structure.

One shortcut, for the large cases: a set pixel whose eight neighbours are all set has ``C = 0`` and is never deleted, so a
sub-iteration loops over the other set pixels only (found with array slices; the decision itself stays the scalar loop)."""
import numpy as np
from scipy import ndimage

SKELETON_COLS = 8
EIGHT = np.ones((3, 3), dtype=bool)
ULP = 4                                    # values 6 and 7: within 4 ulp of the f64 formula


def _candidates(img: np.ndarray) -> list:
    """Flat indices (into the padded image) of the set pixels with at least one unset 8-neighbour."""
    h, w = img.shape[0] - 2, img.shape[1] - 2
    c = img[1:-1, 1:-1] != 0
    inner = c.copy()
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            inner &= img[dy:dy + h, dx:dx + w] != 0
    ys, xs = np.nonzero(c & ~inner)
    return ((ys + 1) * img.shape[1] + xs + 1).tolist()


def sub_iteration(a: bytearray, h: int, w: int, sub: int) -> int:
    """One Guo-Hall sub-iteration on the padded byte image ``a`` ((h + 2) x (w + 2), row-major), in place: every pixel is decided on
    the state before it, then the deleted ones are cleared.  Returns how many were deleted."""
    s = w + 2
    kill = []
    for i in _candidates(np.frombuffer(bytes(a), dtype=np.uint8).reshape(h + 2, s)):
        p2, p3, p4, p5 = a[i - s] != 0, a[i - s + 1] != 0, a[i + 1] != 0, a[i + s + 1] != 0
        p6, p7, p8, p9 = a[i + s] != 0, a[i + s - 1] != 0, a[i - 1] != 0, a[i - s - 1] != 0
        C = int((not p2) and (p3 or p4)) + int((not p4) and (p5 or p6)) + int((not p6) and (p7 or p8)) + int((not p8) and (p9 or p2))
        N1 = int(p9 or p2) + int(p3 or p4) + int(p5 or p6) + int(p7 or p8)
        N2 = int(p2 or p3) + int(p4 or p5) + int(p6 or p7) + int(p8 or p9)
        N = min(N1, N2)
        if sub == 0:
            m = (p6 or p7 or (not p9)) and p8
        else:
            m = (p2 or p3 or (not p5)) and p4
        if C == 1 and 2 <= N <= 3 and not m:
            kill.append(i)
    for i in kill:
        a[i] = 0
    return len(kill)


def thin(mask: np.ndarray):
    """(skeleton [H, W] bool, pairs of sub-iterations run, the last -- which deleted nothing -- included)."""
    mask = np.asarray(mask, dtype=bool)
    h, w = mask.shape
    a = bytearray(np.pad(mask, 1).astype(np.uint8).tobytes())
    pairs = 0
    while True:
        pairs += 1
        if sub_iteration(a, h, w, 0) + sub_iteration(a, h, w, 1) == 0:
            break
    return np.frombuffer(bytes(a), dtype=np.uint8).reshape(h + 2, w + 2)[1:-1, 1:-1] != 0, pairs


def components(mask: np.ndarray) -> int:
    return int(ndimage.label(np.asarray(mask, dtype=bool), structure=EIGHT)[1])


def holes(mask: np.ndarray) -> int:
    """4-connected components of the background that do not reach the outside of the frame."""
    return int(ndimage.label(~np.pad(np.asarray(mask, dtype=bool), 1))[1]) - 1


def counts(sk: np.ndarray):
    """(n, n4, nd, ends, branches) of a set of skeleton pixels ``sk`` [H, W] bool, by scalar loops over its pixels."""
    h, w = sk.shape
    g = np.pad(sk, 1).tolist()

    def at(x, y):
        return g[y + 1][x + 1]

    n = n4 = nd = ends = branches = 0
    ys, xs = np.nonzero(sk)
    for x, y in zip(xs.tolist(), ys.tolist()):
        n += 1
        n4 += int(at(x + 1, y)) + int(at(x, y + 1))
        if at(x + 1, y + 1) and not at(x + 1, y) and not at(x, y + 1):
            nd += 1
        if at(x - 1, y + 1) and not at(x - 1, y) and not at(x, y + 1):
            nd += 1
        ring = [at(x, y - 1), at(x + 1, y - 1), at(x + 1, y), at(x + 1, y + 1), at(x, y + 1), at(x - 1, y + 1), at(x - 1, y), at(x - 1, y - 1)]
        if sum(ring) == 1:
            ends += 1
        if sum(1 for j in range(8) if not ring[j] and ring[(j + 1) % 8]) >= 3:
            branches += 1
    return n, n4, nd, ends, branches


class Reference:
    """The skeleton and the 8-connected components of one mask, computed once; :meth:`values` per contour start."""

    def __init__(self, mask: np.ndarray):
        self.mask = np.asarray(mask, dtype=bool)
        self.skeleton, self.pairs = thin(self.mask)
        self.labels, self.n = ndimage.label(self.mask, structure=EIGHT)

    def integers(self, sx: int, sy: int):
        """(n, n4, nd, ends, branches, Npix) of the component that contains the pixel (sx, sy), as Python ints."""
        lab = int(self.labels[sy, sx])
        assert lab > 0, (sx, sy)
        k = self.labels == lab
        return counts(self.skeleton & k) + (int(k.sum()),)

    def values(self, sx: int, sy: int, um: float) -> np.ndarray:
        n, n4, nd, ends, branches, npix = self.integers(sx, sy)
        return np.array([n, n4, nd, ends, branches, npix, (np.float64(n4) + np.sqrt(np.float64(2.0)) * np.float64(nd)) * um,
                         np.float64(npix) / np.float64(n) * um], dtype=np.float64)

    def starts(self):
        """The raster-first pixel (sx, sy) of every component that is NOT nested in a hole -- the components that have an
        external contour --, in label order (= raster order of the first pixel)."""
        outside = ndimage.label(~np.pad(self.mask, 1))[0]                      # 4-connected background; label of the padding = outside
        outside = outside == outside[0, 0]
        near = ndimage.binary_dilation(outside, structure=EIGHT)[1:-1, 1:-1]
        out = []
        for lab in range(1, self.n + 1):
            k = self.labels == lab
            if (k & near).any():
                ys, xs = np.nonzero(k)
                out.append((int(xs[0]), int(ys[0])))
        return out


def compare(got, want):
    """Differences between a kernel row and :meth:`Reference.values`, as messages: values 0-5 equal as integers, 6-7 within 4 ulp."""
    got = np.asarray(got, dtype=np.float64)
    bad = []
    for j in range(6):
        if got[j] != want[j] or got[j] != int(got[j]):
            bad.append(f"value {j}: {got[j]!r} != {want[j]!r}")
    for j in (6, 7):
        if not abs(got[j] - want[j]) <= ULP * np.spacing(abs(want[j])):
            bad.append(f"value {j}: {got[j]!r} vs {want[j]!r} ({abs(got[j] - want[j]) / np.spacing(abs(want[j])):.3g} ulp)")
    return bad
