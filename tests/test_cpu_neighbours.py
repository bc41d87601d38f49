"""The parts of the neighbour statistics that need no GPU: the reference of ``tests/neighbour_ref.py`` against hand-made answers and
against itself (brute force vs the index transform, symmetry), the two limits of ``csrc/neighbours.hip`` against the scenes made to
exceed them, the host offsets, the setting's parsing and refusals, and the rows of ``neighbours_results.csv``."""
import csv
import io
import math

import numpy as np
import pytest

import neighbour_cases as NC
import neighbour_ref as NR

SCENES = NC.by_name()
SMALL = [n for n, s in SCENES.items() if s.masks.shape[0] <= 8 and n != "combs"]


@pytest.fixture(scope="module")
def d2s():
    """name -> d2 matrix, computed once and shared."""
    return {n: NR.d2_matrix(s.masks) for n, s in SCENES.items()}


# ---------------------------------------------------------------------------------------------------------------- reference
@pytest.mark.parametrize("name", list(SCENES))
def test_known_answers_and_symmetry(name, d2s):
    s, d2 = SCENES[name], d2s[name]
    M = s.masks.shape[0]
    for (a, b), v in s.known_d2.items():
        assert d2[a][b] == v, (a, b, d2[a][b], v)
    for a in range(M):
        assert d2[a][a] == -1
        for b in range(a):
            assert d2[a][b] == d2[b][a] and isinstance(d2[a][b], int)
    tab = NR.table(s.masks, s.group, s.r2, d2=d2)
    for a, i in s.known_nearest.items():
        assert tab[a][1] == i, (a, tab[a])
    for a, i in s.known_group_nearest.items():
        assert tab[a][3] == i, (a, tab[a])


@pytest.mark.parametrize("name", SMALL)
def test_index_transform_equals_brute_force(name, d2s):
    s, d2 = SCENES[name], d2s[name]
    M = s.masks.shape[0]
    for a in range(M):
        for b in range(M):
            if a != b:
                assert d2[a][b] == NR.pair_d2_brute(s.masks[a], s.masks[b]), (a, b)


def test_index_transform_equals_brute_force_on_random_scenes():
    for seed in NC.RANDOM_SEEDS[:6]:
        s = NC.random_scene(seed)
        d2 = NR.d2_matrix(s.masks)
        M = s.masks.shape[0]
        rng = np.random.default_rng(seed)
        for a, b in rng.integers(0, M, (25, 2)).tolist():
            if a != b:
                assert d2[a][b] == NR.pair_d2_brute(s.masks[a], s.masks[b]), (seed, a, b)


def test_the_scenes_are_what_their_names_say(d2s):
    s = SCENES["disc_in_hole"]
    assert not (s.masks[0] & s.masks[1]).any() and d2s["disc_in_hole"][0][1] > 2           # disjoint, though the box contains it
    b = NR.tight_boxes(s.masks)
    assert b[0][0] < b[1][0] and b[0][1] < b[1][1] and b[0][2] > b[1][2] and b[0][3] > b[1][3]
    t = NR.table(SCENES["tie_lower_index_wins"].masks)
    assert t[1][:2] == [100, 2]
    s = SCENES["empty_among"]
    t = NR.table(s.masks, s.group, s.r2)
    assert t[1] == [-1, -1, -1, -1, 0, 0] and t[3] == [-1, -1, -1, -1, 0, 0] and t[2][2:4] == [-1, -1] and t[0][4:] == [0, 0]
    assert NR.table(SCENES["single"].masks, None, 100) == [[-1, -1, -1, -1, 0, 0]]
    assert NR.table(SCENES["single"].masks) == [[-1, -1, -1, -1, 0, -1]]
    s = SCENES["groups_differ"]
    t = NR.table(s.masks, s.group, s.r2)
    assert t[0][:4] == [16, 1, 256, 2] and t[0][5] == 1
    # the pruning traps: the boxes meet (or all but meet) where the pixels are far apart
    s = SCENES["interlocking_ls"]
    b = NR.tight_boxes(s.masks)
    assert max(b[0][0], b[1][0]) <= min(b[0][2], b[1][2]) and max(b[0][1], b[1][1]) <= min(b[0][3], b[1][3]) and d2s["interlocking_ls"][0][1] == 169
    s = SCENES["gap_not_nearest"]
    b = NR.tight_boxes(s.masks).astype(np.int64)

    def gap(p, q):
        gy, gx = max(0, q[0] - p[2], p[0] - q[2]), max(0, q[1] - p[3], p[1] - q[3])
        return int(gy * gy + gx * gx)
    assert gap(b[0], b[1]) < gap(b[0], b[2]) == d2s["gap_not_nearest"][0][2] < d2s["gap_not_nearest"][0][1]
    # the radius exactly on, and one below, the pair's distance
    assert NR.table(SCENES["radius_169"].masks, None, 169)[0][5] == 1 and NR.table(SCENES["radius_168"].masks, None, 168)[0][5] == 0
    assert d2s["long_row"][0][1] > 2 ** 31
    # touching counts: overlapping, 4-adjacent and diagonal pairs count, a gap of one pixel does not
    t = NR.table(SCENES["adjacency"].masks)
    assert [r[4] for r in t] == [1, 1, 1, 1]
    assert NR.table(SCENES["overlap_contained"].masks)[0][4] == 2


def test_scenes_exceed_the_kernel_limits():
    lds, cand = NC.parse_limits()
    assert (lds, cand) == (NC.LDS_POINTS, NC.CAND_LIST)
    comb = SCENES["combs"].masks
    assert len(NR.border(comb[0])) > 3 * lds and len(NR.border(comb[0])) == int(comb[0].sum())
    # both sides of the staging limit decide something: a mask near the comb's first rows and one far down its raster order
    assert int(comb[0][:19].sum()) < lds < int(comb[0][:100].sum())
    for name in ("many_small", "many_small_all_within"):
        m = SCENES[name].masks
        assert m.shape[0] - 1 > 2 * cand and all(1 <= int(x.sum()) <= 4 for x in m)
    # ... and with the large radius every mask stays a candidate to the end
    s = SCENES["many_small_all_within"]
    assert all(r[5] == NC.N_SMALL - 1 for r in NR.table(s.masks, s.group, s.r2))


def test_frames_are_not_word_aligned():
    for s in SCENES.values():
        assert s.hw[1] % 32 != 0 or s.name.startswith("many_small"), s.name        # (128 x 160: the size the scene is stated at)
        assert s.masks.dtype == bool
    for name in ("adjacency", "overlap_contained", "edges_corners"):
        b = NR.tight_boxes(SCENES[name].masks)
        assert any(x0 >> 5 != x1 >> 5 or (x0 & 31) in (0, 31) for _, x0, _, x1 in b.tolist() if x0 >= 0), name


# ---------------------------------------------------------------------------------------------------------------- host side
def test_host_offsets():
    from deepemia_amd.maskset import Neighbours, neighbour_offsets
    off = neighbour_offsets(np.array([5, 0, 7, 1], dtype=np.int32))
    assert off.dtype == np.int64 and off.tolist() == [0, 5, 5, 12, 13]
    assert neighbour_offsets(np.zeros(0)).tolist() == [0]
    assert neighbour_offsets([3, -1, 2]).tolist() == [0, 3, 3, 5]                 # (a count is never negative)
    big = neighbour_offsets(np.full(3, 2 ** 31 - 1, dtype=np.int32))
    assert big[-1] == 3 * (2 ** 31 - 1)
    t = np.array([[2 ** 40 + 5, 1, -1, -1, 0, -1]], dtype=np.int64)
    s = np.array([[3, 2 ** 33, 7]], dtype=np.int64)
    t2, s2 = Neighbours.from_i32(t.view(np.int32), s.view(np.int32).reshape(-1))
    assert np.array_equal(t2, t) and np.array_equal(s2, s)


def test_setting_parsing_and_refusals():
    from deepemia_amd.functions.inference import neighbour_r2, neighbours_setting
    assert neighbours_setting({}) == (False, None) and neighbours_setting(None) == (False, None)
    assert neighbours_setting({"neighbour_statistics": True}) == (True, None)
    assert neighbours_setting({"neighbour_statistics": True, "neighbour_radius": 3}) == (True, 3.0)
    assert neighbours_setting({"neighbour_statistics": False, "neighbour_radius": 0}) == (False, 0.0)
    for bad in ("true", 1, 0, None, 1.0):
        with pytest.raises(ValueError, match="neighbour_statistics"):
            neighbours_setting({"neighbour_statistics": bad})
    for bad in (-1, -0.5, float("nan"), float("inf"), "3", True, [3]):
        with pytest.raises(ValueError, match="neighbour_radius"):
            neighbours_setting({"neighbour_statistics": True, "neighbour_radius": bad})
    assert neighbour_r2(None, 1.0) == -1
    assert neighbour_r2(13.0, 1.0) == 169 and neighbour_r2(12.999, 1.0) == 168 and neighbour_r2(0.0, 0.5) == 0
    assert neighbour_r2(2.5, 0.5) == 25 and neighbour_r2(1.0, 0.37) == math.floor((1.0 / 0.37) ** 2)


def test_pipeline_settings_carry_the_setting(tmp_path, monkeypatch):
    import yaml

    from deepemia_amd.functions.inference import PipelineSettings
    from deepemia_amd.utils import config as C
    (tmp_path / "datasets").mkdir()
    (tmp_path / "config.yaml").write_text(yaml.safe_dump({"paths": {}, "inference_settings": {}}))
    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(tmp_path))
    for inf, want in (({}, (False, None)), ({"neighbour_statistics": True, "neighbour_radius": 2.5}, (True, 2.5))):
        (tmp_path / "datasets" / "ds.yaml").write_text(yaml.safe_dump({"inference_overrides": inf}))
        C.reset_cache()
        st = PipelineSettings("ds")
        assert st.neighbours == want and st.descriptors == ()
    (tmp_path / "datasets" / "ds.yaml").write_text(yaml.safe_dump({"inference_overrides": {"neighbour_statistics": "yes"}}))
    C.reset_cache()
    with pytest.raises(ValueError):
        PipelineSettings("ds")
    C.reset_cache()


def test_neighbour_rows():
    from deepemia_amd.functions.inference import NEIGHBOUR_CSV_HEADER, neighbour_rows, write_neighbours
    assert NEIGHBOUR_CSV_HEADER == ["Instance_ID", "Class", "Class_Name", "Pixels", "Centroid x", "Centroid y", "Nearest neighbour",
                                    "Nearest distance", "Nearest same-class neighbour", "Nearest same-class distance", "Touching neighbours",
                                    "Neighbours within radius", "Detected scale bar", "File name"]
    table = np.array([[2, 1, -1, -1, 1, -1], [2, 0, 2 ** 33 + 1, 3, 1, -1], [-1, -1, -1, -1, 0, -1], [7, 1, 2 ** 33 + 1, 1, 0, -1]], dtype=np.int64)
    sums = np.array([[4, 10, 21], [1, 7, 7], [0, 0, 0], [3, 2 ** 40, 5]], dtype=np.int64)
    um = 0.37
    rows = neighbour_rows("a.tif", [0, 1, 0, 1], ["pore", "throat"], table, sums, um, "12")
    assert [r[0] for r in rows] == ["a.tif_1", "a.tif_2", "a.tif_4"]                # the empty instance has no row; ids keep counting
    assert all(len(r) == len(NEIGHBOUR_CSV_HEADER) for r in rows)
    assert rows[0] == ["a.tif_1", 0, "pore", 4, (10 / 4) * um, (21 / 4) * um, "a.tif_2", math.sqrt(2) * um, None, None, 1, None, "12", "a.tif"]
    assert rows[1][6:10] == ["a.tif_1", math.sqrt(2) * um, "a.tif_4", math.sqrt(2 ** 33 + 1) * um]
    assert rows[2][3:6] == [3, (2 ** 40 / 3) * um, (5 / 3) * um] and rows[2][2] == "throat"
    assert all(isinstance(r[3], int) and isinstance(r[10], int) for r in rows)
    # a class beyond the names, a radius that was asked for, pixels as the unit
    table[:, 5] = [0, 2, 0, 1]
    rows = neighbour_rows("b.png", [5, 1, 0, 1], ["pore", "throat"], table, sums, 1.0)
    assert rows[0][2] == "class_5" and [r[11] for r in rows] == [0, 2, 1] and rows[0][12] == "0" and rows[0][7] == math.sqrt(2)
    assert neighbour_rows("c.png", [], ["pore"], np.zeros((0, 6), dtype=np.int64), np.zeros((0, 3), dtype=np.int64), 1.0) == []


def test_write_neighbours(tmp_path):
    from deepemia_amd.functions.inference import NEIGHBOUR_CSV_HEADER, write_neighbours
    rows = {"b.png": [["b.png_1", 0, "pore", 4, 2.5, 5.25, None, None, None, None, 0, None, "0", "b.png"]],
            "a.png": [["a.png_1", 1, "throat", 1, 7.0, 7.0, "a.png_2", 1.0, None, None, 1, 3, "0", "a.png"]]}
    path = write_neighbours(str(tmp_path), ["b.png", "skipped.png", "a.png"], rows)
    got = list(csv.reader(io.StringIO(open(path, newline="").read(), newline="")))
    assert got == [NEIGHBOUR_CSV_HEADER, ["b.png_1", "0", "pore", "4", "2.5", "5.25", "", "", "", "", "0", "", "0", "b.png"],
                   ["a.png_1", "1", "throat", "1", "7.0", "7.0", "a.png_2", "1.0", "", "", "1", "3", "0", "a.png"]]


def test_exports_and_abi_version():
    from deepemia_amd import _lib
    header = (NC.SOURCE.parents[2] / "include" / "deepemia_hip.h").read_text()
    for name in ("demia_mask_neighbours", "demia_crop_neighbours"):
        assert name in _lib.EXPORTS and f"int {name}(" in header
    assert len(_lib.EXPORTS["demia_mask_neighbours"][1]) == 13 and len(_lib.EXPORTS["demia_crop_neighbours"][1]) == 15
