"""A literal reference of the agglomerate statistics (``demia_mask_agglomerates``; definitions: ``include/deepemia_hip.h``) on dense
NumPy masks, with Python-int results.  It shares nothing with the kernels: no borders, no boxes, no bit matrix.

``d2`` is ``neighbour_ref.d2_matrix`` (``pair_d2_brute`` for a spot check), links are a plain double loop, components a scalar
union-find (checked against ``scipy.sparse.csgraph.connected_components``), the moments of a component come from
``np.logical_or.reduce`` over its members and ``own`` from its definition.
"""
import numpy as np

import neighbour_ref as NR

try:
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
except ImportError:                                   # the union-find alone
    connected_components = None


def link_matrix(masks: np.ndarray, group=None, l2: int = 2, d2=None) -> list:
    """[M][M] bools: link(a, b)."""
    masks = np.asarray(masks) != 0
    M = masks.shape[0]
    d2 = NR.d2_matrix(masks) if d2 is None else d2
    n = [int(m.sum()) for m in masks]
    group = [0] * M if group is None else [int(g) for g in group]
    out = [[False] * M for _ in range(M)]
    for a in range(M):
        for b in range(M):
            out[a][b] = a != b and n[a] > 0 and n[b] > 0 and group[a] == group[b] and 0 <= d2[a][b] <= l2
    return out


def degrees(links: list) -> list:
    return [sum(1 for v in row if v) for row in links]


def labels(masks: np.ndarray, links: list) -> list:
    """[M] Python ints: the smallest index of m's component; -1 for a mask without a pixel.  A scalar union-find."""
    masks = np.asarray(masks) != 0
    M = masks.shape[0]
    parent = list(range(M))

    def find(i):
        while parent[i] != i:
            i = parent[i]
        return i
    for a in range(M):
        for b in range(a + 1, M):
            if links[a][b]:
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    roots = [find(m) for m in range(M)]
    smallest = {}
    for m, r in enumerate(roots):
        smallest[r] = min(smallest.get(r, m), m)
    out = [smallest[r] if masks[m].any() else -1 for m, r in enumerate(roots)]
    if connected_components is not None and M:
        _, comp = connected_components(csr_matrix(np.array(links, dtype=np.int8).reshape(M, M)), directed=False)
        for a in range(M):
            for b in range(M):
                if out[a] >= 0 and out[b] >= 0:
                    assert (comp[a] == comp[b]) == (out[a] == out[b])
    return out


def moments(mask: np.ndarray) -> list:
    """[6] Python ints N, Sx, Sy, Sxx, Syy, Sxy of a dense mask, absolute pixel coordinates."""
    ys, xs = np.nonzero(np.asarray(mask) != 0)
    ys, xs = [int(v) for v in ys], [int(v) for v in xs]
    return [len(ys), sum(xs), sum(ys), sum(x * x for x in xs), sum(y * y for y in ys), sum(x * y for x, y in zip(xs, ys))]


def own(masks: np.ndarray, links: list) -> list:
    """[M][6]: the moments of the pixels of m that belong to no mask b < m with link(b, m)."""
    masks = np.asarray(masks) != 0
    out = []
    for m in range(masks.shape[0]):
        keep = masks[m].copy()
        for b in range(m):
            if links[b][m]:
                keep &= ~masks[b]
        out.append(moments(keep))
    return out


def components(masks: np.ndarray, lab: list) -> dict:
    """label -> (members ascending, moments of the OR of the members)."""
    masks = np.asarray(masks) != 0
    out = {}
    for root in sorted({v for v in lab if v >= 0}):
        mem = [m for m, v in enumerate(lab) if v == root]
        out[root] = (mem, moments(np.logical_or.reduce(masks[mem], axis=0)))
    return out


def pack_links(links: list) -> list:
    """The bit matrix [M][ceil(M / 32)] of Python ints, as the entries lay it out."""
    M = len(links)
    rows = []
    for a in range(M):
        words = [0] * ((M + 31) // 32)
        for b in range(M):
            if links[a][b]:
                words[b >> 5] |= 1 << (b & 31)
        rows.append(words)
    return rows


def everything(masks: np.ndarray, group=None, l2: int = 2, d2=None) -> dict:
    """links (packed), degree, label, own -- what the entries write -- as Python ints."""
    lk = link_matrix(masks, group, l2, d2)
    return {"links": pack_links(lk), "degree": degrees(lk), "label": labels(masks, lk), "own": own(masks, lk)}
