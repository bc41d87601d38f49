"""The skeleton reference (``tests/skeleton_ref.py``) against the known answers of the definition and against the invariants of a
thinning, the ``inference_settings.skeleton_descriptors`` setting, the CSV row widths of all eight on/off combinations, and the host
sizing function of the crop entry's second scratch -- everything that needs no GPU."""
import numpy as np
import pytest

import skeleton_cases as SC
import skeleton_ref as SR

TRACE_WORDS = 8192          # the trace's large LDS buffer, in words (csrc/contours.hip)


@pytest.fixture(scope="module")
def cases():
    return SC.by_name()


@pytest.fixture(scope="module")
def refs(cases):
    return {name: SR.Reference(c.mask) for name, c in cases.items()}


def test_known_answers(cases, refs):
    assert len(SC.KNOWN) == 9
    for name in SC.KNOWN:
        c, ref = cases[name], refs[name]
        starts = ref.starts()
        assert len(starts) == c.contours == len(c.known) == 1
        assert ref.integers(*starts[0])[:5] == c.known[0], name
    # of the 2 x 2 block the top-right pixel survives
    assert np.argwhere(refs["k_block2x2"].skeleton).tolist() == [[3, 4]]
    assert refs["k_ellipse140x60"].pairs == SC.ELLIPSE_PAIRS
    v = refs["k_ring18_9"].values(*refs["k_ring18_9"].starts()[0], 0.5)
    assert v[6] == (40 + np.sqrt(2.0) * 34) * 0.5 and v[7] == 756 / 74 * 0.5 and v[5] == 756
    # a junction has one branch point and three ends, a plus four
    for name, ends in (("junction_T", 3), ("junction_Y", 3), ("k_plus41", 4)):
        assert refs[name].integers(*refs[name].starts()[0])[3:5] == (ends, 1), name


def _check_invariants(mask, skel, what):
    assert not (skel & ~mask).any(), what                                 # a subset of the mask
    labels, n = SR.ndimage.label(mask, structure=SR.EIGHT)
    assert SR.components(skel) == n, what                                 # no component split, merged or lost
    assert SR.holes(skel) == SR.holes(mask), what
    if n:
        assert (np.bincount(labels[skel], minlength=n + 1)[1:] >= 1).all(), what      # at least one pixel per component
    again, pairs = SR.thin(skel)
    assert pairs == 1 and np.array_equal(again, skel), what              # a skeleton is its own skeleton


def test_invariants_on_the_cases(cases, refs):
    for name, c in cases.items():
        _check_invariants(c.mask, refs[name].skeleton, name)
        if c.contours >= 0:
            assert len(refs[name].starts()) == c.contours, name


def test_invariants_on_random_masks():
    rng = np.random.default_rng(20)
    for k in range(240):                                                 # noise, fills 0.2 .. 0.95, frames up to 13 x 13
        h, w = (int(v) for v in rng.integers(1, 14, size=2))
        m = rng.random((h, w)) < rng.uniform(0.2, 0.95)
        _check_invariants(m, SR.thin(m)[0], ("noise", k))
    for k in range(40):                                                  # smoothed-noise blobs up to 60 x 60
        h, w = (int(v) for v in rng.integers(20, 61, size=2))
        f = SR.ndimage.gaussian_filter(rng.random((h, w)), sigma=float(rng.uniform(1.5, 4.0)))
        m = f > np.quantile(f, float(rng.uniform(0.3, 0.7)))
        _check_invariants(m, SR.thin(m)[0], ("blob", k))


def test_setting_default_off_per_dataset_bool_only():
    from deepemia_amd.functions import inference as inf
    assert inf.descriptors_setting({}) == () and inf.descriptors_setting(None) == ()
    assert inf.descriptors_setting({"skeleton_descriptors": True}) == ("skeleton",)
    assert inf.descriptors_setting({"skeleton_descriptors": False, "inscribed_descriptors": True}) == ("inscribed",)
    # table order, whatever the order of the keys
    assert inf.descriptors_setting({"skeleton_descriptors": True, "inscribed_descriptors": True, "shape_descriptors": True}) == ("shape", "inscribed", "skeleton")
    for bad in (1, 0, "true", "yes", None, [True], 1.0):
        with pytest.raises(ValueError, match="skeleton_descriptors"):
            inf.descriptors_setting({"skeleton_descriptors": bad})
    assert inf.SKELETON_CSV_HEADER == ["Skeleton length", "Skeleton mean width", "Skeleton end points", "Skeleton branch points",
                                       "Skeleton pixels"]
    assert not set(inf.SKELETON_CSV_HEADER) & set(inf.CSV_HEADER + inf.SHAPE_CSV_HEADER + inf.INSCRIBED_CSV_HEADER)


def test_row_widths_of_all_eight_combinations():
    from deepemia_amd.functions import inference as inf
    shape = np.arange(100.0, 110.0)
    insc = np.array([401.0, 30.0, 31.0, 1257.0, 87661.0, 20.5, 4.25, 1.0005])
    skel = np.array([74.0, 40.0, 34.0, 2.0, 1.0, 756.0, 44.04, 5.108])
    widths = []
    plain = inf.measurement_rows("img.tif", [1], [[dict(area=50.0, perimeter=30.0, values=np.arange(12.0))]], ["a", "b"], 5.0)[0]
    for with_skel in (False, True):
        for with_shape, with_insc in ((False, False), (False, True), (True, False), (True, True)):
            rec = dict(area=50.0, perimeter=30.0, values=np.arange(12.0))
            if with_shape:
                rec["shape"] = shape
            if with_insc:
                rec["inscribed"] = insc
            if with_skel:
                rec["skeleton"] = skel
            rows = inf.measurement_rows("img.tif", [1], [[rec, dict(rec, area=1.0)]], ["a", "b"], 5.0)      # the second: below the area gate
            assert len(rows) == 1
            header = inf.CSV_HEADER + [col for name, (cols, _) in inf.DESCRIPTOR_CSV.items() if name in rec for col in cols]
            assert len(header) == len(rows[0])
            widths.append(len(rows[0]))
            assert rows[0][:20] == plain
            if with_shape:
                assert rows[0][20:27] == list(shape[3:10])
            if with_insc:
                at = 27 if with_shape else 20
                assert rows[0][at:at + 6] == [20.5, 30.0, 31.0, 4.25, 1.0005, 1257.0]
            if with_skel:
                # Skeleton length, mean width, end points, branch points, pixels
                assert rows[0][-5:] == [44.04, 5.108, 2.0, 1.0, 74.0] and all(type(x) is float for x in rows[0][-5:])
    assert sorted(widths) == [20, 25, 26, 27, 31, 32, 33, 38]


def test_rows_of_every_subset_follow_the_table():
    """Each family a record holds appends its columns of ``DESCRIPTOR_CSV`` behind the 20, at the offset the table order gives it,
    whatever the order of the record's keys; the table is the one of ``maskset.FAMILIES``."""
    import itertools

    from deepemia_amd.functions import inference as inf
    from deepemia_amd.maskset import FAMILIES
    assert list(inf.DESCRIPTOR_CSV) == list(FAMILIES) == ["shape", "inscribed", "skeleton"]
    assert [FAMILIES[n].cols for n in FAMILIES] == [10, 8, 8] and [FAMILIES[n].words for n in FAMILIES] == [False, True, True]
    assert [inf.DESCRIPTOR_CSV[n][1] for n in FAMILIES] == [(3, 4, 5, 6, 7, 8, 9), (5, 1, 2, 6, 7, 3), (6, 7, 3, 4, 0)]
    assert (inf.SHAPE_CSV_HEADER, inf.INSCRIBED_CSV_HEADER, inf.SKELETON_CSV_HEADER) == tuple(inf.DESCRIPTOR_CSV[n][0] for n in FAMILIES)
    values = {n: 1000.0 * (i + 1) + np.arange(float(FAMILIES[n].cols)) for i, n in enumerate(FAMILIES)}
    subsets = [s for k in range(4) for s in itertools.combinations(FAMILIES, k)]
    assert len(subsets) == 8
    for subset in subsets:
        rec = dict(area=50.0, perimeter=30.0, values=np.arange(12.0))
        for name in reversed(subset):                                    # keys in reverse table order
            rec[name] = values[name]
        row, = inf.measurement_rows("img.tif", [1], [[rec]], ["a", "b"], 5.0)
        assert len(row) == 20 + sum(len(inf.DESCRIPTOR_CSV[n][0]) for n in subset)
        at = 20
        for name in subset:                                              # (combinations keeps the table order)
            header, index = inf.DESCRIPTOR_CSV[name]
            assert len(header) == len(index) and row[at:at + len(header)] == [float(values[name][k]) for k in index]
            at += len(header)
        assert at == len(row)


# ------------------------------------------------------------------------------------------------------ the second scratch
def _restated(room, H, W):
    """Per mask: the region of its ROOM grown by one ring and clipped to the frame, rows x word columns, padded by one more row /
    word on every side: ONE such buffer when it exceeds TRACE_WORDS, nothing otherwise."""
    room = np.asarray(room, dtype=np.int64).reshape(-1, 4)
    ry0, ry1 = np.maximum(room[:, 0] - 1, 0), np.minimum(room[:, 2] + 1, H - 1)
    wx0, wx1 = np.maximum(room[:, 1] - 1, 0) >> 5, np.minimum(room[:, 3] + 1, W - 1) >> 5
    pn = (ry1 - ry0 + 1 + 2) * (wx1 - wx0 + 1 + 2)
    return np.where((room[:, 0] >= 0) & (pn > TRACE_WORDS), pn, 0), pn


def _native(name, room, H, W):
    from deepemia_amd import _lib
    lib = _lib.load()
    room = np.ascontiguousarray(room, dtype=np.int32).reshape(-1, 4)
    off = np.full(max(len(room), 1), -7, dtype=np.int64)
    total = int(getattr(lib, name)(room.ctypes.data, len(room), H, W, off.ctypes.data))
    return off[:len(room)], total


def test_second_scratch_equals_the_restated_rule_and_is_half_the_tracers():
    H, W = 700, 4000
    g = np.random.default_rng(4)
    n = 300
    y0, x0 = g.integers(0, H, n), g.integers(0, W, n)
    y1, x1 = np.minimum(y0 + g.integers(0, H, n), H - 1), np.minimum(x0 + g.integers(0, W, n), W - 1)
    room = np.stack([y0, x0, y1, x1], axis=1)
    room[g.random(n) < 0.1] = -1
    fixed = [[0, 0, H - 1, W - 1], [-1, -1, -1, -1], [0, 0, 0, 0], [H - 1, W - 1, H - 1, W - 1],
             [10, 64, 261, 959], [10, 64, 262, 959]]                      # the last two: 8192 padded words (LDS) and one row more
    room = np.concatenate([room, np.asarray(fixed)])
    off, total = _native("demia_crop_skeleton_scratch", room, H, W)
    lens, pn = _restated(room, H, W)
    assert np.array_equal(off, np.concatenate(([0], np.cumsum(lens)[:-1])))
    assert total == int(lens.sum()) and (lens > 0).sum() > 50 and (lens[room[:, 0] >= 0] == 0).sum() > 20
    assert lens[-6] == (H + 2) * ((W + 31) // 32 + 2) and pn[-2:].tolist() == [8192, 8224] and lens[-2:].tolist() == [0, 8224]
    off_t, total_t = _native("demia_crop_contour_scratch", room, H, W)     # the tracer's share: two such regions for the same masks
    assert total_t == 2 * total and np.array_equal(off_t, 2 * off)
    assert _native("demia_crop_skeleton_scratch", np.zeros((0, 4), np.int32), H, W)[1] == 0
