"""The descriptor table (``maskset.FAMILIES``): families are independent of one another and of the order they are launched in.

Three masks in a 40 x 70 frame (the width is no multiple of 32): a solid blob, five separate 3 x 3 squares (more contours than the four
slots: the fetch falls back) and an empty mask.  Every subset of the table, through every path that takes ``descriptors``, gives each
family the bits it has when it is requested alone on planes, and leaves points, area, perimeter and the 12 values as they are without
any family."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UM = 0.37
H, W = 40, 70
BASE_KEYS = {"start", "area", "perimeter", "points", "values"}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _squares(n):
    m = np.zeros((H, W), dtype=bool)
    for y, x in [(3, 4), (3, 40), (20, 62), (33, 10), (30, 35)][:n]:
        m[y:y + 3, x:x + 3] = True
    return m


def _blob():
    m = np.zeros((H, W), dtype=bool)
    m[6:31, 12:55] = True
    m[10:26, 55:66] = True                                               # across the word boundaries at 32 and 64
    return m


@pytest.fixture(scope="module")
def ops(gpu_device):
    from deepemia_amd.maskset import MaskOps
    ops = MaskOps(gpu_device)
    ops.set_frame_width(W)
    return ops


@pytest.fixture(scope="module")
def masks():
    return np.stack([_blob(), _squares(5), np.zeros((H, W), dtype=bool)])


@pytest.fixture(scope="module")
def table():
    from deepemia_amd.maskset import FAMILIES
    assert list(FAMILIES) == ["shape", "inscribed", "skeleton"]
    return FAMILIES


@pytest.fixture(scope="module")
def alone(ops, masks, table):
    """The records without any family, and per family the records with that family alone, on planes: computed once, left unchanged."""
    planes = ops.from_dense(masks)
    out = {(): ops.contours(planes, max_contours=16, um_pix=UM)}
    for name in table:
        out[name] = ops.contours(planes, max_contours=16, um_pix=UM, descriptors=(name,))
    assert [len(rs) for rs in out[()]] == [1, 5, 0]
    return out


def _paths(ops, masks, subset):
    """name of the path -> records of ``masks`` with the families ``subset``."""
    from deepemia_amd.cropset import CropMaskSet, CropPlanes, crop_contours
    planes = ops.from_dense(masks)
    cset = CropMaskSet.from_planes(ops, planes, W)
    out = {"planes": ops.contours(planes, max_contours=16, um_pix=UM, descriptors=subset),
           "crop_direct": cset.contours(max_contours=16, um_pix=UM, descriptors=subset),
           "crop": crop_contours(cset, CropPlanes(ops, (H, W), chunk=2), UM, max_contours=16, descriptors=subset)[0]}
    cs = ops.trace(planes, max_contours=16, keep_words=True)
    for name in reversed(subset):                                        # launched in REVERSE table order, the 12 values last
        cs.launch(name, UM, slots=4)
    cs.launch_measure(UM, slots=4)
    cs.fetch(with_points=True)
    out["reverse"] = cs.records(um_pix=UM, descriptors=subset)
    return out


def test_every_subset_through_every_path_equals_each_family_alone(ops, masks, table, alone):
    subsets = [s for k in range(len(table) + 1) for s in itertools.combinations(table, k)]
    assert len(subsets) == 8
    for subset in subsets:
        for path, recs in _paths(ops, masks, subset).items():
            what = (subset, path)
            assert [len(rs) for rs in recs] == [1, 5, 0], what
            for m, rs in enumerate(recs):
                for c, r in enumerate(rs):
                    assert set(r) == BASE_KEYS | set(subset), what       # exactly the requested keys
                    base = alone[()][m][c]
                    assert r["start"] == base["start"] and np.array_equal(r["points"], base["points"]), what
                    for key in ("area", "perimeter", "values"):
                        assert (_bits(r[key]) == _bits(base[key])).all(), what + (key,)
                    for name in subset:
                        want = alone[name][m][c][name]
                        assert r[name].shape == want.shape == (table[name].cols,) and (_bits(r[name]) == _bits(want)).all(), what + (name, m, c)


def test_an_unknown_family_is_a_value_error(ops, masks):
    from deepemia_amd.cropset import CropMaskSet, CropPlanes, crop_contours, trace_chunks
    from deepemia_amd.maskset import families
    planes = ops.from_dense(masks)
    cset = CropMaskSet.from_planes(ops, planes, W)
    cp = CropPlanes(ops, (H, W), chunk=2)
    cs = ops.trace(planes, max_contours=16, keep_words=True)
    bad = ("shape", "hull")
    for call in (lambda: families(bad),
                 lambda: ops.contours(planes, max_contours=16, um_pix=UM, descriptors=bad),
                 lambda: cset.contours(max_contours=16, um_pix=UM, descriptors=bad),
                 lambda: crop_contours(cset, cp, UM, max_contours=16, descriptors=bad),
                 lambda: list(trace_chunks(cset, cp, max_contours=16, um_pix=UM, descriptors=bad)),
                 lambda: cs.launch("hull", UM),
                 lambda: cs.launch_all(UM, True, bad),
                 lambda: cs.descriptor("hull", UM),
                 lambda: cs.records(um_pix=UM, descriptors=bad)):
        with pytest.raises(ValueError, match="hull"):
            call()
    assert cs.launched == {}                                             # launch_all checks the names before it enqueues anything


def test_host_views_are_none_exactly_when_the_fetch_fell_back(ops, masks, table, alone):
    few = np.stack([_blob(), _squares(4), np.zeros((H, W), dtype=bool)])
    for ms, fallback in ((masks[1:2], True), (few, False)):
        cs = ops.trace(ops.from_dense(ms), max_contours=16, keep_words=True)
        cs.launch_all(UM, True, tuple(table), slots=4)
        cs.fetch(with_points=True)
        assert list(cs.launched) == list(table) and (cs.max_count > 4) == fallback
        for name, st in cs.launched.items():
            assert (st.host is None) == fallback, name
            assert st.slots == 4 and tuple(st.dev.shape) == (len(ms), 4, table[name].cols)
        if fallback:                                                     # on demand: the five squares' values of the shared reference
            for name in table:
                got = cs.records(um_pix=UM, descriptors=(name,))[0]
                assert all((_bits(r[name]) == _bits(a[name])).all() for r, a in zip(got, alone[name][1])), name


def test_a_family_with_too_few_slots_falls_back_alone(ops, table):
    """Three contours, the 12 values and ``inscribed`` in four slots, ``shape`` in two: the shape view is dropped, and the inscribed
    view behind it in the float64 block is still read at its own offset."""
    ms = np.stack([_squares(3), _blob()])
    planes = ops.from_dense(ms)
    cs = ops.trace(planes, max_contours=16, keep_words=True)
    cs.launch_measure(UM, slots=4)
    cs.launch("inscribed", UM, slots=4)
    cs.launch("shape", UM, slots=2)
    cs.fetch(with_points=True)
    assert cs.max_count == 3 and cs.launched["shape"].host is None and cs.launched["inscribed"].host is not None
    carried = cs.launched["inscribed"].host
    assert carried.shape == (2, 3, table["inscribed"].cols)
    assert (_bits(carried) == _bits(cs.launched["inscribed"].dev.cpu().numpy()[:, :3])).all()
    shape = cs.descriptor("shape", UM)                                   # on demand, over the three slots in use
    assert shape.shape == (2, 3, table["shape"].cols) and (_bits(shape[:, :2]) == _bits(cs.launched["shape"].dev.cpu().numpy())).all()
