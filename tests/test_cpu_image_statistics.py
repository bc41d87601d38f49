"""The table of the per-image statistics stages (``IMAGE_STATISTICS`` in ``functions/inference.py``) without a GPU: its entries
against the literals of the two stages, the layout of the ride and its decoding by entry, the one writer behind the no-device path
of ``write_measurements``, the merge of the ranks' rows by stage name, and a third entry that costs nothing but its entry."""
import csv
import io
import os
from types import SimpleNamespace

import numpy as np
import pytest

NEIGHBOUR_HEADER = ["Instance_ID", "Class", "Class_Name", "Pixels", "Centroid x", "Centroid y", "Nearest neighbour", "Nearest distance",
                    "Nearest same-class neighbour", "Nearest same-class distance", "Touching neighbours", "Neighbours within radius",
                    "Detected scale bar", "File name"]
AGGLOMERATE_HEADER = ["Agglomerate_ID", "Members", "Member ids", "Class counts", "Links", "Mean coordination", "Pixels", "Member pixels",
                      "Centroid x", "Centroid y", "Equivalent diameter", "Radius of gyration", "Major extent", "Minor extent", "Orientation",
                      "Detected scale bar", "File name"]
IMAGES = ["b.png", "skipped.png", "a.png"]
# the inputs of test_write_neighbours (tests/test_cpu_neighbours.py) and test_write_agglomerates (tests/test_cpu_agglomerates.py)
NEIGHBOUR_ROWS = {"b.png": [["b.png_1", 0, "pore", 4, 2.5, 5.25, None, None, None, None, 0, None, "0", "b.png"]],
                  "a.png": [["a.png_1", 1, "throat", 1, 7.0, 7.0, "a.png_2", 1.0, None, None, 1, 3, "0", "a.png"]]}
_AROW = ["b.png_A1", 2, "b.png_1 b.png_2", "pore:2", 1, 1.0, 7, 8, 1.0, 1.5, 2.0, 0.5, 3.0, 0.0, 45.0, "0", "b.png"]
AGGLOMERATE_ROWS = {"b.png": [_AROW], "a.png": [["a.png_A1"] + _AROW[1:16] + ["a.png"]]}


def _csv_bytes(header, rows_by_image):
    """What the two writers before the table wrote: the header, then every image's rows in the order of ``IMAGES``."""
    buf = io.StringIO(newline="")
    w = csv.writer(buf)
    w.writerow(header)
    for name in IMAGES:
        for r in rows_by_image.get(name, []):
            w.writerow(r)
    return buf.getvalue().encode()


def _folder(tmp_path):
    """An image folder whose images are never opened, an output folder, and one measurement row per instance-bearing image."""
    inp, out = tmp_path / "in", tmp_path / "out"
    inp.mkdir()
    out.mkdir()
    for name in IMAGES:
        (inp / name).write_bytes(b"")
    dedup = {"b.png": {"masks": None}, "a.png": {"masks": None}}                 # (skipped.png: the image loop skipped it)
    rows = {name: [[f"{name}_1", 0, "pore"] + [1.5] * 12 + [None] * 3 + ["0", name]] for name in dedup}
    return inp, out, dedup, rows


def _no_device_run(I, inp, out, dedup, rows, statistics, statistic_rows):
    """Rank 0's output section for the stages: ``ops`` None and no image, since every image comes with its rows."""
    I.write_measurements(None, dedup, str(inp), str(out), SimpleNamespace(thing_classes=["pore", "throat"]), "ds", rows_by_image=rows,
                         statistics=statistics, statistic_rows_by_image=statistic_rows)
    return I.write_statistics(str(out), statistics, IMAGES, statistic_rows)


def test_table_consistency(tmp_path, monkeypatch):
    import yaml

    from deepemia_amd.functions import inference as I
    from deepemia_amd.utils import config as C
    assert list(I.IMAGE_STATISTICS) == ["neighbours", "agglomerates"]
    want = {"neighbours": ("neighbour_statistics", "neighbours_results.csv", NEIGHBOUR_HEADER, "neighbour_radius"),
            "agglomerates": ("agglomerate_statistics", "agglomerates_results.csv", AGGLOMERATE_HEADER, "agglomerate_gap")}
    for name, stage in I.IMAGE_STATISTICS.items():
        key, filename, header, length = want[name]
        assert (stage.name, stage.key, stage.filename, stage.header) == (name, key, filename, header)
        assert stage.setting({}).enabled is False and stage.setting({key: True}).enabled is True
        for bad in ("yes", 1, None):
            with pytest.raises(ValueError) as e:
                stage.setting({key: bad})
            assert str(e.value) == f"inference_settings.{key} must be true or false, got {bad!r}"
        for bad in (-1, float("inf"), "3", True):
            with pytest.raises(ValueError) as e:
                stage.setting({key: True, length: bad})
            assert str(e.value) == f"inference_settings.{length} must be a finite number >= 0, got {bad!r}"
    assert I.IMAGE_STATISTICS["neighbours"].setting is I.neighbours_setting and I.IMAGE_STATISTICS["agglomerates"].setting is I.agglomerates_setting
    assert not hasattr(I, "NeighbourStage") and not hasattr(I, "AgglomerateStage")
    # PipelineSettings: one setting per entry, all off without a key, and only what was asked for on
    (tmp_path / "datasets").mkdir()
    (tmp_path / "config.yaml").write_text(yaml.safe_dump({"paths": {}, "inference_settings": {}}))
    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(tmp_path))
    for inf, on in (({}, []), ({"agglomerate_statistics": True}, ["agglomerates"]),
                    ({"agglomerate_statistics": True, "neighbour_statistics": True}, ["neighbours", "agglomerates"])):
        (tmp_path / "datasets" / "ds.yaml").write_text(yaml.safe_dump({"inference_overrides": inf}))
        C.reset_cache()
        st = I.PipelineSettings("ds")
        assert list(st.statistics) == list(I.IMAGE_STATISTICS)
        assert [name for name, s in st.statistics.items() if s.enabled] == on
        assert [stage.name for stage, _ in I.enabled_statistics(st.statistics)] == on
    C.reset_cache()
    assert I.enabled_statistics(None) == [] and I.enabled_statistics({}) == []


@pytest.mark.parametrize("M", [0, 1, 3])
def test_ride_layout(M):
    from deepemia_amd.functions import inference as I
    from deepemia_amd.maskset import Agglomerates, Neighbours
    rng = np.random.default_rng(M)
    table = rng.integers(0, 2 ** 40, size=(M, 6), dtype=np.int64)
    table[:, 1], table[:, 3] = (np.arange(M) + 1) % max(M, 1), -1
    sums = rng.integers(1, 2 ** 40, size=(M, 3), dtype=np.int64)
    label, degree = np.zeros(M, dtype=np.int32), rng.integers(0, 5, size=M, dtype=np.int32)
    own = rng.integers(1, 2 ** 50, size=(M, 6), dtype=np.int64)
    extra = np.arange(7, dtype=np.int32)
    # the shapes of Neighbours.ride ([M, 12], [M, 6]) and Agglomerates.ride ([M], [M], [M, 12]) behind one array of the caller's
    nb_ride = [table.view(np.int32).reshape(M, 12), sums.view(np.int32).reshape(M, 6)]
    ag_ride = [label, degree, own.view(np.int32).reshape(M, 12)]
    rides = I.take_rides([extra] + nb_ride + ag_ride, 1, [("neighbours", 2), ("agglomerates", 3)])
    assert list(rides) == ["neighbours", "agglomerates"]
    assert all(a is b for a, b in zip(rides["neighbours"], nb_ride)) and all(a is b for a, b in zip(rides["agglomerates"], ag_ride))
    t2, s2 = Neighbours.from_i32(*rides["neighbours"])
    assert np.array_equal(t2, table) and np.array_equal(s2, sums) and t2.dtype == s2.dtype == np.int64
    l2, d2, o2 = Agglomerates.from_i32(*rides["agglomerates"])
    assert np.array_equal(l2, label) and np.array_equal(d2, degree) and np.array_equal(o2, own) and o2.dtype == np.int64
    # one stage alone, with and without the caller's array
    only = I.take_rides([extra] + ag_ride, 1, [("agglomerates", 3)])
    assert list(only) == ["agglomerates"] and all(a is b for a, b in zip(only["agglomerates"], ag_ride))
    assert all(a is b for a, b in zip(I.take_rides(nb_ride, 0, [("neighbours", 2)])["neighbours"], nb_ride))
    with pytest.raises(AssertionError):
        I.take_rides([extra] + nb_ride + ag_ride, 1, [("neighbours", 2)])          # (arrays nobody asked for)
    # the entries' decoding of their own arrays is the rows functions on the int64 tables
    classes, names, pixels = list(range(M)), ["pore", "throat"], [int(v) for v in own[:, 0]]
    nb, ag = I.IMAGE_STATISTICS["neighbours"], I.IMAGE_STATISTICS["agglomerates"]
    assert nb.decode("a.tif", classes, names, rides["neighbours"], 0.5, "12", pixels, None) == I.neighbour_rows("a.tif", classes, names, table, sums, 0.5, "12")
    got = ag.decode("a.tif", classes, names, rides["agglomerates"], 0.5, "12", pixels, None)
    assert got == I.agglomerate_rows("a.tif", classes, names, label, degree, own, pixels, 0.5, "12") and len(got) == min(M, 1)


def test_writer_and_no_device_path(tmp_path):
    from deepemia_amd.functions import inference as I
    inp, out, dedup, rows = _folder(tmp_path)
    statistics = I.statistics_setting({"neighbour_statistics": True, "neighbour_radius": 3, "agglomerate_statistics": True})
    stat_rows = {"neighbours": dict(NEIGHBOUR_ROWS), "agglomerates": dict(AGGLOMERATE_ROWS)}
    paths = _no_device_run(I, inp, out, dedup, rows, statistics, stat_rows)
    assert paths == [str(out / "neighbours_results.csv"), str(out / "agglomerates_results.csv")]
    assert (out / "neighbours_results.csv").read_bytes() == _csv_bytes(NEIGHBOUR_HEADER, NEIGHBOUR_ROWS)
    assert (out / "agglomerates_results.csv").read_bytes() == _csv_bytes(AGGLOMERATE_HEADER, AGGLOMERATE_ROWS)
    assert stat_rows == {"neighbours": NEIGHBOUR_ROWS, "agglomerates": AGGLOMERATE_ROWS}        # rows that came in are left as they are
    # the wrappers under the old names are that writer
    assert open(I.write_neighbours(str(tmp_path), IMAGES, NEIGHBOUR_ROWS), "rb").read() == _csv_bytes(NEIGHBOUR_HEADER, NEIGHBOUR_ROWS)
    assert open(I.write_agglomerates(str(tmp_path), IMAGES, AGGLOMERATE_ROWS), "rb").read() == _csv_bytes(AGGLOMERATE_HEADER, AGGLOMERATE_ROWS)
    # the measurements: the given rows in the folder's order, the skipped image without a row
    got = list(csv.reader(io.StringIO(open(out / "measurements_results.csv", newline="").read(), newline="")))
    assert got[0] == I.CSV_HEADER and [r[-1] for r in got[1:]] == [f for f in os.listdir(inp) if f in dedup]
    # a stage that is off writes nothing, whatever rows there are
    for f in list(out.iterdir()):
        f.unlink()
    off = I.statistics_setting({"agglomerate_statistics": True})
    assert _no_device_run(I, inp, out, dedup, rows, off, stat_rows) == [str(out / "agglomerates_results.csv")]
    assert sorted(f.name for f in out.iterdir()) == ["agglomerates_results.csv", "measurements_results.csv"]
    for f in list(out.iterdir()):
        f.unlink()
    assert _no_device_run(I, inp, out, dedup, rows, None, {}) == [] and [f.name for f in out.iterdir()] == ["measurements_results.csv"]


def test_rank_merge():
    from deepemia_amd.functions import inference as I
    rank0 = {"neighbours": {"b.png": NEIGHBOUR_ROWS["b.png"]}, "agglomerates": {"b.png": AGGLOMERATE_ROWS["b.png"]}}
    rank1 = {"neighbours": {"a.png": NEIGHBOUR_ROWS["a.png"], "empty.png": []}}
    merged = I.merge_statistic_rows(rank0, rank1)
    assert merged is rank0
    assert merged == {"neighbours": {"b.png": NEIGHBOUR_ROWS["b.png"], "a.png": NEIGHBOUR_ROWS["a.png"], "empty.png": []},
                      "agglomerates": {"b.png": AGGLOMERATE_ROWS["b.png"]}}
    assert rank1 == {"neighbours": {"a.png": NEIGHBOUR_ROWS["a.png"], "empty.png": []}}
    # a rank 0 without an image of its own takes the other ranks' stages; a stage nobody enabled stays absent
    assert I.merge_statistic_rows({}, rank1) == rank1 and I.merge_statistic_rows({}, {}) == {}
    assert "agglomerates" not in I.merge_statistic_rows({"neighbours": {}}, rank1)


def test_a_third_entry_costs_one_entry(tmp_path, monkeypatch):
    from deepemia_amd.functions import inference as I
    stub = I.ImageStatistic("stub", "stub_statistics", lambda inf: SimpleNamespace(enabled=bool((inf or {}).get("stub_statistics", False))),
                            "stub_results.csv", ["Value"], None, None)
    monkeypatch.setitem(I.IMAGE_STATISTICS, "stub", stub)
    statistics = I.statistics_setting({"stub_statistics": True, "neighbour_statistics": True})
    assert list(statistics) == ["neighbours", "agglomerates", "stub"]
    assert [stage.name for stage, _ in I.enabled_statistics(statistics)] == ["neighbours", "stub"]
    inp, out, dedup, rows = _folder(tmp_path)
    stat_rows = I.merge_statistic_rows({"neighbours": {"b.png": NEIGHBOUR_ROWS["b.png"]}, "stub": {"b.png": [[1], [2]]}},
                                       {"neighbours": {"a.png": NEIGHBOUR_ROWS["a.png"]}, "stub": {"a.png": [["three"]]}})
    paths = _no_device_run(I, inp, out, dedup, rows, statistics, stat_rows)
    assert paths == [str(out / "neighbours_results.csv"), str(out / "stub_results.csv")]
    assert (out / "stub_results.csv").read_bytes() == b"Value\r\n1\r\n2\r\nthree\r\n"
    assert (out / "neighbours_results.csv").read_bytes() == _csv_bytes(NEIGHBOUR_HEADER, NEIGHBOUR_ROWS)
    assert not (out / "agglomerates_results.csv").exists()
