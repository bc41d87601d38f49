"""The inscribed-descriptor reference (``tests/inscribed_ref.py``) against brute force and the known answers of the definition, the
``inference_settings.inscribed_descriptors`` setting, and the CSV row widths -- everything that needs no GPU."""
import numpy as np
import pytest

import inscribed_cases as IC
import inscribed_ref as IR


@pytest.fixture(scope="module")
def cases():
    return IC.by_name()


def test_edt_reference_equals_brute_force_on_the_small_cases(cases):
    small = [c for c in cases.values() if c.small]
    assert len(small) >= 10
    for c in small:
        assert np.array_equal(IR.d2_edt(c.mask), IR.d2_brute(c.mask)), c.name
    rng = np.random.default_rng(5)
    for k in range(12):                                                  # random masks, fills 0.5 .. 1.0, frames up to 33 x 33
        h, w = (int(v) for v in rng.integers(1, 34, size=2))
        m = rng.random((h, w)) < 0.5 + 0.5 * k / 11
        assert np.array_equal(IR.d2_edt(m), IR.d2_brute(m)), (k, h, w)


def test_known_answers(cases):
    for name in IC.KNOWN:
        c = cases[name]
        ref = IR.Reference(c.mask)
        starts = ref.starts()
        assert len(starts) == c.contours == len(c.known) == 1
        assert ref.integers(*starts[0]) == c.known[0], name
        if c.small:
            assert IR.Reference(c.mask, brute=True).integers(*starts[0]) == c.known[0], name
    v = IR.Reference(cases["disc"].mask).values(30, 10, 0.5)
    assert v[5] == 2.0 * np.sqrt(401.0) * 0.5 and v[6] == np.sqrt(87661 / 1257) * 0.5 and abs(v[7] - 1.0) < 2e-3


def test_contour_counts_and_nested_component(cases):
    for c in cases.values():
        if c.contours >= 0:
            assert len(IR.Reference(c.mask).starts()) == c.contours, c.name
    nested, ring = IR.Reference(cases["nested_in_ring"].mask), IR.Reference(cases["ring"].mask)
    assert nested.n == 2 and len(nested.starts()) == 1
    (sx, sy), = nested.starts()
    # the nested pixels are nobody's K, and a background pixel separates them from the rim: the ring's values are those of the ring alone
    assert nested.integers(sx, sy) == ring.integers(sx, sy) == IC.by_name()["ring"].known[0]
    # the tie rule: the raster-first of a plateau of centres
    assert IR.Reference(cases["rect_even"].mask).integers(5, 4)[:3] == (36, 10, 9)
    assert IR.Reference(cases["rect_odd"].mask).integers(5, 4)[:3] == (36, 10, 9)


def test_setting_default_off_per_dataset_bool_only():
    from deepemia_amd.functions import inference as inf
    assert inf.descriptors_setting({}) == () and inf.descriptors_setting(None) == ()
    assert inf.descriptors_setting({"inscribed_descriptors": True}) == ("inscribed",)
    assert inf.descriptors_setting({"inscribed_descriptors": False, "shape_descriptors": True}) == ("shape",)
    for bad in (1, 0, "true", "yes", None, [True], 1.0):
        with pytest.raises(ValueError, match="inscribed_descriptors"):
            inf.descriptors_setting({"inscribed_descriptors": bad})
    assert len(inf.INSCRIBED_CSV_HEADER) == 6 and not set(inf.INSCRIBED_CSV_HEADER) & set(inf.CSV_HEADER + inf.SHAPE_CSV_HEADER)


def test_row_widths_20_26_27_33():
    from deepemia_amd.functions import inference as inf
    shape = np.arange(100.0, 110.0)
    insc = np.array([401.0, 30.0, 31.0, 1257.0, 87661.0, 20.5, 4.25, 1.0005])
    for with_shape, with_insc, width in ((False, False, 20), (False, True, 26), (True, False, 27), (True, True, 33)):
        rec = dict(area=50.0, perimeter=30.0, values=np.arange(12.0))
        if with_shape:
            rec["shape"] = shape
        if with_insc:
            rec["inscribed"] = insc
        small = dict(rec, area=1.0)                                      # below the area gate: no row
        rows = inf.measurement_rows("img.tif", [1], [[rec, small]], ["a", "b"], 5.0)
        assert len(rows) == 1 and len(rows[0]) == width
        header = inf.CSV_HEADER + (inf.SHAPE_CSV_HEADER if with_shape else []) + (inf.INSCRIBED_CSV_HEADER if with_insc else [])
        assert len(header) == width
        assert rows[0][:20] == inf.measurement_rows("img.tif", [1], [[dict(area=50.0, perimeter=30.0, values=np.arange(12.0))]], ["a", "b"], 5.0)[0]
        if with_shape:
            assert rows[0][20:27] == list(shape[3:10])
        if with_insc:
            # Inscribed diameter, centre x, centre y, RMS boundary distance, Inscribed ratio, Component pixels
            assert rows[0][-6:] == [20.5, 30.0, 31.0, 4.25, 1.0005, 1257.0]
            assert all(type(x) is float for x in rows[0][-6:])
