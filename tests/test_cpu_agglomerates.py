"""The agglomerate statistics without a GPU: the reference of ``tests/agglomerate_ref.py`` against answers known by hand and its
own invariants on the scenes of ``tests/agglomerate_cases.py``, then the host side -- the setting and its refusals,
``agglomerate_l2``, ``agglomerate_rows`` / ``write_agglomerates`` on hand-made tables, the limits parsed from the source and the
new symbols in the header and in ``_lib.py``."""
import csv
import io
import math

import numpy as np
import pytest

import agglomerate_cases as AC
import agglomerate_ref as AR
import neighbour_ref as NR

SCENES = AC.by_name()


@pytest.fixture(scope="module")
def refs():
    return {n: AR.everything(s.masks, s.group, s.l2) for n, s in SCENES.items()}


def _parts(label):
    out = {}
    for m, v in enumerate(label):
        if v >= 0:
            out.setdefault(v, set()).add(m)
    return sorted(out.values(), key=min)


# ---------------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (4, 12), (33, 2)])
def test_rectangle_moments_are_the_textbook_ones(w, h):
    m = np.zeros((1, 40, 70), dtype=bool)
    m[0, 9:9 + h, 30:30 + w] = True
    n, sx, sy, sxx, syy, sxy = AR.moments(m[0])
    assert n == w * h and (n * sxx - sx * sx) * 12 == n * n * (w * w - 1) and (n * syy - sy * sy) * 12 == n * n * (h * h - 1)
    assert n * sxy - sx * sy == 0
    from deepemia_amd.functions.inference import agglomerate_rows
    ref = AR.everything(m)
    row = agglomerate_rows("r.png", [0], ["p"], ref["label"], ref["degree"], ref["own"], [n], 1.0)[0]
    assert row[1] == 1 and row[4] == 0 and row[6] == row[7] == n
    assert row[8] == 30 + (w - 1) / 2 and row[9] == 9 + (h - 1) / 2
    assert row[11] == pytest.approx(math.sqrt((w * w - 1) / 12 + (h * h - 1) / 12), rel=1e-12)
    if w != h:
        assert row[14] == (0.0 if w > h else 90.0)
        assert row[12] == pytest.approx(4 * math.sqrt((max(w, h) ** 2 - 1) / 12), rel=1e-12)
        assert row[13] == pytest.approx(4 * math.sqrt((min(w, h) ** 2 - 1) / 12), rel=1e-12, abs=1e-12)


def test_two_rectangles_in_diagonal_contact_are_one_component():
    m = np.zeros((2, 40, 70), dtype=bool)
    m[0, 5:8, 10:17] = True
    m[1, 8:11, 17:24] = True
    ref = AR.everything(m, None, 2)
    assert NR.pair_d2_brute(m[0], m[1]) == 2
    assert ref["label"] == [0, 0] and ref["degree"] == [1, 1] and ref["links"] == [[2], [1]]
    assert [sum(c) for c in zip(*ref["own"])] == AR.moments(m[0] | m[1]) and ref["own"][0][0] == ref["own"][1][0] == 21


def test_known_partitions(refs):
    for name, s in SCENES.items():
        assert _parts(refs[name]["label"]) == sorted(s.known_parts, key=min), name


def test_partition_invariants(refs):
    for name, s in SCENES.items():
        r = refs[name]
        M = s.masks.shape[0]
        lab = r["label"]
        lk = AR.link_matrix(s.masks, s.group, s.l2)
        assert all(lk[a][b] == lk[b][a] and not lk[a][a] for a in range(M) for b in range(M)), name
        assert all((lab[m] >= 0) == bool(s.masks[m].any()) for m in range(M)), name
        assert all(lab[lab[m]] == lab[m] <= m for m in range(M) if lab[m] >= 0), name
        assert all(lab[a] == lab[b] for a in range(M) for b in range(M) if lk[a][b]), name
        assert sum(r["degree"]) % 2 == 0
        comps = AR.components(s.masks, lab)
        assert sorted(m for mem, _ in comps.values() for m in mem) == [m for m in range(M) if lab[m] >= 0], name
        for root, (mem, mom) in comps.items():
            assert [sum(r["own"][m][j] for m in mem) for j in range(6)] == mom, (name, root)
        if s.group is None:
            assert sum(o[0] for o in r["own"]) == int(np.logical_or.reduce(s.masks, axis=0).sum()), name


def test_scenes_hit_what_they_are_for(refs):
    assert AC.parse_limits() == {"LDS_POINTS": AC.LDS_POINTS, "NEAR": AC.NEAR, "OWN_LIST": AC.OWN_LIST, "LABEL_LDS": AC.LABEL_LDS, "MAX_M": AC.MAX_M, "MAX_HW": AC.MAX_HW}
    comb = SCENES["long_border"].masks[0]
    assert len(NR.border(comb)) == int(comb.sum()) > AC.LDS_POINTS
    assert all(s.masks.shape[1] <= 96 and s.masks.shape[2] <= 200 for s in SCENES.values())
    assert SCENES["last_column"].masks[:, :, -1].any() and SCENES["last_column"].masks.shape[2] % 32
    d2 = NR.d2_matrix(SCENES["pairs_l2_2"].masks)
    assert [d2[a][a + 1] for a in (0, 2, 4, 6)] == [1, 2, 4, 5]
    assert NR.d2_matrix(SCENES["disc_in_hole"].masks)[0][1] > 5
    assert NR.d2_matrix(SCENES["interleaved_l2_2"].masks)[0][1] == 4
    assert refs["many_lower"]["degree"][70] == 70 > AC.OWN_LIST and 0 < refs["many_lower"]["own"][70][0] < int(SCENES["many_lower"].masks[70].sum())
    ov = SCENES["overlaps"].masks
    assert int((ov[2] & ov[3] & ov[4]).sum()) > 0
    assert 64 < SCENES["chain_cap_64"].masks.shape[0] and SCENES["chain_cap_64"].cap == 64
    assert refs["classes_any"]["own"][7][0] < int(SCENES["classes_any"].masks[7].sum()) == refs["classes_same"]["own"][7][0]
    for M in (33, 65):
        lk = refs[f"row_word_edges_{M}"]["links"]
        assert lk[31][1] == 1 and lk[32][0] == 1 << 31 and (M == 33 or (lk[63][2] == 1 and lk[64][1] == 1 << 31))


# ---------------------------------------------------------------------------------------------------------------- host side
def test_setting_parsing_and_refusals():
    from deepemia_amd.functions.inference import agglomerate_l2, agglomerates_setting
    assert agglomerates_setting({}) == (False, None, "any") and agglomerates_setting(None) == (False, None, "any")
    assert agglomerates_setting({"agglomerate_statistics": True}) == (True, None, "any")
    assert agglomerates_setting({"agglomerate_statistics": True, "agglomerate_gap": 3, "agglomerate_link": "same_class"}) == (True, 3.0, "same_class")
    for bad in ("true", 1, 0, None, 1.0):
        with pytest.raises(ValueError, match="agglomerate_statistics"):
            agglomerates_setting({"agglomerate_statistics": bad})
    for bad in (-1, -0.5, float("nan"), float("inf"), "3", True, [3]):
        with pytest.raises(ValueError, match="agglomerate_gap"):
            agglomerates_setting({"agglomerate_statistics": True, "agglomerate_gap": bad})
    for bad in ("all", "", None, 1, True, "Same_class"):
        with pytest.raises(ValueError, match="agglomerate_link"):
            agglomerates_setting({"agglomerate_statistics": True, "agglomerate_link": bad})
    assert agglomerate_l2(None, 1.0) == 2 and agglomerate_l2(0.0, 1.0) == 2 and agglomerate_l2(1.0, 1.0) == 2
    assert agglomerate_l2(2.0, 1.0) == 4 and agglomerate_l2(2.2361, 1.0) == 5 and agglomerate_l2(2.236, 1.0) == 4
    assert agglomerate_l2(2.5, 0.5) == 25 and agglomerate_l2(1.0, 0.37) == math.floor((1.0 / 0.37) ** 2)


def test_pipeline_settings_carry_the_setting(tmp_path, monkeypatch):
    import yaml

    from deepemia_amd.functions.inference import PipelineSettings
    from deepemia_amd.utils import config as C
    (tmp_path / "datasets").mkdir()
    (tmp_path / "config.yaml").write_text(yaml.safe_dump({"paths": {}, "inference_settings": {}}))
    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(tmp_path))
    for inf, want in (({}, (False, None, "any")), ({"agglomerate_statistics": True, "agglomerate_gap": 2.5}, (True, 2.5, "any"))):
        (tmp_path / "datasets" / "ds.yaml").write_text(yaml.safe_dump({"inference_overrides": inf}))
        C.reset_cache()
        st = PipelineSettings("ds")
        assert st.agglomerates == want and st.neighbours == (False, None)
    (tmp_path / "datasets" / "ds.yaml").write_text(yaml.safe_dump({"inference_overrides": {"agglomerate_link": "nearby"}}))
    C.reset_cache()
    with pytest.raises(ValueError):
        PipelineSettings("ds")
    C.reset_cache()


def test_host_views():
    from deepemia_amd.maskset import Agglomerates
    lab = np.array([0, -1, 0], dtype=np.int32)
    deg = np.array([1, 0, 1], dtype=np.int32)
    own = np.array([[3, 2 ** 33, 7, 2 ** 50, 9, -1], [0] * 6, [1, 2, 3, 4, 5, 6]], dtype=np.int64)
    l2, d2, o2 = Agglomerates.from_i32(lab, deg, own.view(np.int32).reshape(-1))
    assert np.array_equal(l2, lab) and np.array_equal(d2, deg) and np.array_equal(o2, own) and o2.dtype == np.int64


def test_agglomerate_rows():
    from deepemia_amd.functions.inference import AGGLOMERATE_CSV_HEADER, agglomerate_rows
    assert AGGLOMERATE_CSV_HEADER == ["Agglomerate_ID", "Members", "Member ids", "Class counts", "Links", "Mean coordination", "Pixels",
                                      "Member pixels", "Centroid x", "Centroid y", "Equivalent diameter", "Radius of gyration",
                                      "Major extent", "Minor extent", "Orientation", "Detected scale bar", "File name"]
    # 0 and 3: 2 x 2 squares at (0 .. 1, 0 .. 1) and (1 .. 2, 1 .. 2), sharing pixel (1, 1); 1: empty; 2: a single pixel at (9, 5); 4 links to 2
    label = np.array([0, -1, 2, 0, 2], dtype=np.int32)
    degree = np.array([1, 0, 1, 1, 1], dtype=np.int32)
    own = np.array([[4, 2, 2, 2, 2, 1], [0] * 6, [1, 5, 9, 25, 81, 45], [3, 5, 5, 9, 9, 8], [1, 6, 9, 36, 81, 54]], dtype=np.int64)
    um = 0.5
    rows = agglomerate_rows("a.tif", [0, 0, 1, 1, 7], ["pore", "throat"], label, degree, own, [4, 0, 1, 4, 1], um, "12")
    assert [r[0] for r in rows] == ["a.tif_A1", "a.tif_A2"] and all(len(r) == len(AGGLOMERATE_CSV_HEADER) for r in rows)
    r = rows[0]
    n, sx, sy, sxx, syy, sxy = 7, 7, 7, 11, 11, 9
    mxx, myy, mxy = (n * sxx - sx * sx) / n ** 2, (n * syy - sy * sy) / n ** 2, (n * sxy - sx * sy) / n ** 2
    root = math.sqrt(((mxx - myy) / 2) ** 2 + mxy ** 2)
    assert r[:8] == ["a.tif_A1", 2, "a.tif_1 a.tif_4", "pore:1 throat:1", 1, 1.0, 7, 8]
    assert r[8:] == [1.0 * um, 1.0 * um, math.sqrt(28 / math.pi) * um, math.sqrt(mxx + myy) * um, 4 * math.sqrt((mxx + myy) / 2 + root) * um,
                     4 * math.sqrt(max((mxx + myy) / 2 - root, 0.0)) * um, 45.0, "12", "a.tif"]
    assert rows[1][:8] == ["a.tif_A2", 2, "a.tif_3 a.tif_5", "throat:1 class_7:1", 1, 1.0, 2, 2]
    assert rows[1][14] == 0.0 and rows[1][13] == 0.0 and rows[1][9] == 9.0 * um
    assert all(isinstance(r[k], int) for r in rows for k in (1, 4, 6, 7))
    # sums beyond 2^53 stay exact: Python ints, one division
    big = np.array([[2 ** 20, 2 ** 34, 2 ** 34, 2 ** 49, 2 ** 49, 2 ** 48]], dtype=np.int64)
    row = agglomerate_rows("b.png", [0], ["p"], [0], [0], big, [2 ** 20], 1.0)[0]
    assert row[8] == 2.0 ** 14 and row[11] == math.sqrt(2 * ((2 ** 69 - 2 ** 68) / 2 ** 40)) and row[15] == "0"
    assert agglomerate_rows("c.png", [], ["p"], np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros((0, 6), dtype=np.int64), [], 1.0) == []


def test_write_agglomerates(tmp_path):
    from deepemia_amd.functions.inference import AGGLOMERATE_CSV_HEADER, write_agglomerates
    row = ["b.png_A1", 2, "b.png_1 b.png_2", "pore:2", 1, 1.0, 7, 8, 1.0, 1.5, 2.0, 0.5, 3.0, 0.0, 45.0, "0", "b.png"]
    rows = {"b.png": [row], "a.png": [["a.png_A1"] + row[1:16] + ["a.png"]]}
    path = write_agglomerates(str(tmp_path), ["b.png", "skipped.png", "a.png"], rows)
    assert path.endswith("agglomerates_results.csv")
    got = list(csv.reader(io.StringIO(open(path, newline="").read(), newline="")))
    assert got[0] == AGGLOMERATE_CSV_HEADER and len(got) == 3
    assert got[1] == ["b.png_A1", "2", "b.png_1 b.png_2", "pore:2", "1", "1.0", "7", "8", "1.0", "1.5", "2.0", "0.5", "3.0", "0.0", "45.0", "0", "b.png"]
    assert got[2][0] == "a.png_A1" and got[2][-1] == "a.png"


def test_exports_and_abi_version():
    from deepemia_amd import _lib
    root = AC.CSRC.parents[1]
    header = (root / "include" / "deepemia_hip.h").read_text()
    for name in ("demia_mask_agglomerates", "demia_crop_agglomerates"):
        assert name in _lib.EXPORTS and f"int {name}(" in header
    assert len(_lib.EXPORTS["demia_mask_agglomerates"][1]) == 18 and len(_lib.EXPORTS["demia_crop_agglomerates"][1]) == 20
    assert "have_border" in header and "label_lds_cap" in header
    assert "int demia_abi_version(void) { return 6; }" in (AC.CSRC / "capi.hip").read_text()
    assert "agglomerates.hip" in (AC.CSRC / "Makefile").read_text()
    # one border kernel, in the shared header
    texts = {n: (AC.CSRC / n).read_text() for n in ("neighbours.hip", "agglomerates.hip", "maskborder.h")}
    assert [n for n, t in texts.items() if "void mask_border_kernel(" in t] == ["maskborder.h"]
    assert all('#include "maskborder.h"' in texts[n] for n in ("neighbours.hip", "agglomerates.hip"))

