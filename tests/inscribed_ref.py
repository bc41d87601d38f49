"""A reference of the eight values ``demia_mask_inscribed`` / ``demia_crop_inscribed`` write per contour (definition:
``include/deepemia_hip.h``), sharing no code with the kernel: the mask is padded by one zero ring, ``D2`` comes from SciPy's exact
Euclidean feature transform (the INDEX of the nearest background pixel; the squared distance is then integer arithmetic), the
components from ``ndimage.label`` with the 3 x 3 structure.  ``d2_brute`` -- the minimum over ALL background pixels of the padded
array -- checks the transform on small masks."""
import numpy as np
from scipy import ndimage

INSCRIBED_COLS = 8
# values 5-7 are at most four float64 operations on exact integers (convert, multiply / divide, sqrt, multiply), computed once by the
# kernel and once by NumPy: one ulp per operation and side, in case a sqrt is not correctly rounded
REL_TOL = 8 * 2.0 ** -53
EIGHT = np.ones((3, 3), dtype=bool)


def d2_edt(mask: np.ndarray) -> np.ndarray:
    """[H, W] int64: squared distance of every foreground pixel to the nearest background pixel (0 on the background); positions
    outside the frame are background."""
    m = np.pad(np.asarray(mask, dtype=bool), 1)
    iy, ix = ndimage.distance_transform_edt(m, return_distances=False, return_indices=True)
    yy, xx = np.indices(m.shape)
    d2 = (iy.astype(np.int64) - yy) ** 2 + (ix.astype(np.int64) - xx) ** 2
    return np.where(m, d2, 0)[1:-1, 1:-1]


def d2_brute(mask: np.ndarray) -> np.ndarray:
    """:func:`d2_edt` by brute force (small masks)."""
    m = np.pad(np.asarray(mask, dtype=bool), 1)
    by, bx = np.nonzero(~m)
    fy, fx = np.nonzero(m)
    out = np.zeros(m.shape, dtype=np.int64)
    for lo in range(0, len(fy), 256):
        y, x = fy[lo:lo + 256, None].astype(np.int64), fx[lo:lo + 256, None].astype(np.int64)
        out[fy[lo:lo + 256], fx[lo:lo + 256]] = ((y - by[None]) ** 2 + (x - bx[None]) ** 2).min(axis=1)
    return out[1:-1, 1:-1]


class Reference:
    """``D2`` and the 8-connected components of one mask, computed once; :meth:`values` per contour start."""

    def __init__(self, mask: np.ndarray, brute: bool = False):
        self.mask = np.asarray(mask, dtype=bool)
        self.d2 = d2_brute(self.mask) if brute else d2_edt(self.mask)
        self.labels, self.n = ndimage.label(self.mask, structure=EIGHT)

    def integers(self, sx: int, sy: int):
        """(R2, cx, cy, N, SD2) of the component that contains the pixel (sx, sy), as Python ints."""
        lab = int(self.labels[sy, sx])
        assert lab > 0, (sx, sy)
        k = self.labels == lab
        d = np.where(k, self.d2, 0)
        r2 = int(d.max())
        cy, cx = (int(v[0]) for v in np.nonzero(k & (self.d2 == r2)))           # np.nonzero is in raster order
        return r2, cx, cy, int(k.sum()), int(d.sum(dtype=np.int64))

    def values(self, sx: int, sy: int, um: float) -> np.ndarray:
        r2, cx, cy, n, sd2 = self.integers(sx, sy)
        return np.array([r2, cx, cy, n, sd2, 2.0 * np.sqrt(np.float64(r2)) * um, np.sqrt(np.float64(sd2) / np.float64(n)) * um,
                         np.sqrt(np.pi * np.float64(r2) / np.float64(n))], dtype=np.float64)

    def starts(self):
        """The raster-first pixel (sx, sy) of every component that is NOT nested in a hole -- the components that have an
        external contour --, in label order (= raster order of the first pixel)."""
        outside = ndimage.label(~np.pad(self.mask, 1))[0]                      # 4-connected background; label of the padding = outside
        outside = outside == outside[0, 0]
        near = ndimage.binary_dilation(outside, structure=EIGHT)[1:-1, 1:-1]     # pixels that touch the outside background (8-connected)
        out = []
        for lab in range(1, self.n + 1):
            k = self.labels == lab
            if (k & near).any():
                ys, xs = np.nonzero(k)
                out.append((int(xs[0]), int(ys[0])))
        return out


def compare(got, want):
    """Differences between a kernel row and :meth:`Reference.values`, as messages: values 0-4 exactly, 5-7 within ``REL_TOL``."""
    got = np.asarray(got, dtype=np.float64)
    bad = []
    for j in range(5):
        if got[j] != want[j]:
            bad.append(f"value {j}: {got[j]!r} != {want[j]!r}")
    for j in range(5, 8):
        if not abs(got[j] - want[j]) <= REL_TOL * abs(want[j]):
            bad.append(f"value {j}: {got[j]!r} vs {want[j]!r} (rel {abs(got[j] - want[j]) / abs(want[j]):.3g})")
    return bad


def worst_rel(got, want) -> float:
    return max(abs(got[j] - want[j]) / abs(want[j]) for j in range(5, 8))
