"""CPU: the reference of the convex-hull shape descriptors (``tests/shape_ref.py``) against closed forms and against the hull of
``tests/contour_cases.py``; the ``shape_descriptors`` setting; the 20 / 27 columns of ``measurement_rows``."""
import math

import numpy as np
import pytest
import yaml

import contour_cases as CC
import shape_ref as SR

UM = CC.UM


def _close(a, b):
    return abs(a - b) <= SR.REL_TOL * abs(b)


# ----------------------------------------------------------------------------------------------------- reference vs closed forms
@pytest.mark.parametrize("w, h", [(9, 19), (19, 9), (7, 7), (120, 1)])
def test_axis_aligned_rectangle(w, h):
    x0, y0 = 3005, 7
    pts = np.array([[x0, y0], [x0, y0 + h], [x0 + w, y0 + h], [x0 + w, y0]], dtype=np.int32)
    v = SR.shape_values(pts, float(w * h), 2.0 * (w + h), UM)
    assert v[0] == 2 * w * h and v[1] == w * w + h * h and v[2] == 4
    assert _close(v[3], w * h * UM * UM) and _close(v[4], 2 * (w + h) * UM)
    assert v[5] == 1.0 and v[6] == 1.0
    assert _close(v[7], math.hypot(w, h) * UM) and _close(v[8], min(w, h) * UM)
    # both diagonals have F2: the tie rule takes the smallest a = (x0, y0), whose partner is (x0 + w, y0 + h) -- y grows
    # downwards on the screen, so with y upwards that chord points below the x axis: 180 - atan(h / w)
    assert abs(v[9] - (180.0 - math.degrees(math.atan2(h, w)))) <= SR.ANGLE_TOL
    assert SR.farthest_pair(pts)[1:] == ((x0, y0), (x0 + w, y0 + h))


def test_right_triangle():
    a, b = 30, 40
    pts = np.array([[100, 200], [100 + a, 200], [100, 200 + b]], dtype=np.int32)
    v = SR.shape_values(pts, a * b / 2.0, a + b + 50.0, UM)
    assert v[0] == a * b and v[1] == 2500 and v[2] == 3
    assert _close(v[3], a * b / 2 * UM * UM) and _close(v[4], 120 * UM) and v[5] == 1.0 and v[6] == 1.0
    assert _close(v[7], 50 * UM)
    assert _close(v[8], a * b / 50.0 * UM)                            # the height on the hypotenuse, the smallest of the three
    # the hypotenuse from (100, 240) to (130, 200): a < b by (x, y), dy = -40 -> atan2(40, 30)
    assert abs(v[9] - math.degrees(math.atan2(40, 30))) <= SR.ANGLE_TOL


def test_square_rotated_by_45_degrees_on_the_lattice():
    r = 12
    c = np.array([5000, 6000])
    pts = (c + np.array([[r, 0], [0, r], [-r, 0], [0, -r]])).astype(np.int32)
    v = SR.shape_values(pts, 2.0 * r * r, 4 * r * math.sqrt(2), UM)
    assert v[0] == 4 * r * r and v[1] == 4 * r * r and v[2] == 4
    assert _close(v[4], 4 * r * math.sqrt(2) * UM) and _close(v[7], 2 * r * UM) and _close(v[8], r * math.sqrt(2) * UM)
    # the two diagonals tie: the smallest a is the left vertex (-r, 0), its partner the right one -> a horizontal chord
    assert v[9] == 0.0


def test_spur_contour_has_repeated_points():
    pts = SR.spur_contour()
    assert len(np.unique(pts, axis=0)) == len(pts) - 1
    h = SR.hull(pts)
    assert len(h) == 5 and (946, 725) in h and (946, 730) not in h      # the foot of the spur lies inside the hull: no vertex
    v = SR.shape_values(pts, 77.0, 48.0, UM)
    # rectangle 11 x 7 plus the triangle over its top side, height 5
    assert v[0] == 2 * 11 * 7 + 11 * 5 and v[2] == 5
    assert v[1] == max(6 ** 2 + 12 ** 2, 11 ** 2 + 7 ** 2) == 180
    assert v[5] == 77.0 / (v[0] / 2)


def test_degenerate_hulls():
    cases = {c.name: c.points for c in CC.degenerate_cases()}
    v = SR.shape_values(cases["one_point"], 0.0, 0.0, UM)
    assert (v == np.array([0, 0, 1, 0, 0, 0, 0, 0, 0, 0.0])).all()
    v = SR.shape_values(cases["identical5"], 0.0, 0.0, UM)
    assert (v == np.array([0, 0, 1, 0, 0, 0, 0, 0, 0, 0.0])).all()
    v = SR.shape_values(cases["two_horizontal"], 0.0, 180.0, UM)
    assert v[0] == 0 and v[1] == 90 * 90 and v[2] == 2 and v[4] == 180 * UM and v[5] == 0 and v[6] == 1.0 and v[8] == 0 and v[9] == 0
    v = SR.shape_values(cases["collinear6"], 0.0, 1.0, UM)
    assert v[0] == 0 and v[2] == 2 and v[1] == 2 * 35 * 35 and v[8] == 0
    assert abs(v[9] - 135.0) <= SR.ANGLE_TOL                            # x and y grow together: downwards on the screen


# ----------------------------------------------------------------------------------------------------------- hull cross-check
def test_hull_vertex_set_equals_the_scipy_hull():
    pytest.importorskip("scipy")
    for c in CC.generated_cases() + CC.degenerate_cases():
        mine = {(int(x), int(y)) for x, y in SR.hull(c.points)}
        theirs = {(int(x), int(y)) for x, y in CC.hull_vertices(c.points)}
        assert mine == theirs, c.name


def test_hull_area_is_at_least_the_contour_area():
    from oracle import postproc_ref as P
    for c in CC.generated_cases()[:20]:
        v = SR.shape_values(c.points, P.contour_area(c.points), P.arc_length(c.points), UM)
        # (arcLength takes every edge length in float32, relative eps 6e-8: a convex contour's Convexity is 1 to that precision)
        assert 0 < v[5] <= 1.0 + 1e-12 and 0 < v[6] <= 1.0 + 2.0 ** -23 and v[8] <= v[7], c.name


# ------------------------------------------------------------------------------------------------------------------ setting
def _settings(tmp_path, monkeypatch, overrides):
    from deepemia_amd.functions.inference import PipelineSettings
    from deepemia_amd.utils import config as C
    (tmp_path / "datasets").mkdir(exist_ok=True)
    (tmp_path / "config.yaml").write_text(yaml.safe_dump({"paths": {}, "inference_settings": {"confidence_mode": "auto"}}))
    (tmp_path / "datasets" / "ds.yaml").write_text(yaml.safe_dump({"inference_overrides": overrides}))
    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(tmp_path))
    C.reset_cache()
    try:
        return PipelineSettings("ds")
    finally:
        C.reset_cache()


def test_setting_defaults_to_off_and_is_read_per_dataset(tmp_path, monkeypatch):
    from deepemia_amd.functions.inference import descriptors_setting
    assert descriptors_setting({}) == () and descriptors_setting(None) == ()
    assert descriptors_setting({"shape_descriptors": True}) == ("shape",)
    assert _settings(tmp_path, monkeypatch, {"tile_settings": {"tile_size": 256}}).descriptors == ()
    assert _settings(tmp_path, monkeypatch, {"shape_descriptors": True, "mask_frame": "crop_direct"}).descriptors == ("shape",)


@pytest.mark.parametrize("value", ["true", "on", 1, 0, None, [True], 1.0])
def test_setting_accepts_a_bool_only(tmp_path, monkeypatch, value):
    from deepemia_amd.functions.inference import descriptors_setting
    with pytest.raises(ValueError, match="shape_descriptors"):
        descriptors_setting({"shape_descriptors": value})
    with pytest.raises(ValueError, match="shape_descriptors"):
        _settings(tmp_path, monkeypatch, {"shape_descriptors": value})       # raised while the settings are read: no model yet


# --------------------------------------------------------------------------------------------------------------------- rows
def test_rows_have_27_columns_with_shape_records_and_the_same_20_without():
    from deepemia_amd.functions.inference import CSV_HEADER, SHAPE_CSV_HEADER, measurement_rows
    assert len(CSV_HEADER) == 20 and CSV_HEADER[-1] == "File name"
    assert SHAPE_CSV_HEADER == ["Convex area", "Convex perimeter", "Solidity", "Convexity", "Max Feret diameter", "Min Feret diameter",
                                "Feret angle"]
    g = np.random.default_rng(5)
    plain = [[dict(area=50.0, values=g.random(12))], [dict(area=1.0, values=g.random(12)), dict(area=9.0, values=g.random(12))]]
    shaped = [[dict(c, shape=100.0 + np.arange(10.0) + i) for c in cs] for i, cs in enumerate(plain)]
    contrast = [(1.0, 2.0, 3.0), (None, None, None)]
    a = measurement_rows("im.tif", [0, 1], plain, ("pore",), 5.0, contrast, "600")
    b = measurement_rows("im.tif", [0, 1], shaped, ("pore",), 5.0, contrast, "600")
    assert len(a) == len(b) == 2 and all(len(r) == 20 for r in a) and all(len(r) == 27 for r in b)
    assert [r[:20] for r in b] == a
    assert b[0][20:] == [103.0, 104.0, 105.0, 106.0, 107.0, 108.0, 109.0] and b[1][20:] == [104.0, 105.0, 106.0, 107.0, 108.0, 109.0, 110.0]
    assert all(type(x) is float for r in b for x in r[20:])
