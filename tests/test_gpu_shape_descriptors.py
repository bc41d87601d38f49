"""``demia_contour_shape`` -- the convex-hull shape descriptors per contour -- against the exact reference of
``tests/shape_ref.py``, on tables built from plain point lists (``contour_cases.tables_from_points``: no tracer involved), then up
through ``ContourSet`` and the CLI.

Agreement asked of the ten values: 0-2 (S2, F2, k) equal the reference exactly; 3-8 within relative 1e-12 (a handful of correctly
rounded float64 operations on exact integers, about 2e-15; the bound leaves room for libm's sqrt); the angle within 1e-9 degrees.
The size branches of the kernel: 64 lanes (64 / 65), the LDS limit of 256 points (255 / 256 / 257), the rank sort up to 4096
points and the heap sort beyond (4096 / 4097) -- all among ``contour_cases.SIZES``."""
import csv
import io

import numpy as np
import pytest

import contour_cases as CC
import shape_ref as SR

pytestmark = pytest.mark.gpu

UM = CC.UM
COLS = SR.SHAPE_COLS
OUT_FILL = -7.25
OUT_GUARD = 6 * COLS

# generated contour sizes per mask, as test_gpu_contour_measure.py packs them (blocks (m, c % 4) walk slots c and c + 4: scratch-sized
# -> LDS-sized, LDS-sized -> heap-sorted, both sides of the LDS limit in one loop); the other cases follow as masks of their own
PACKED = ((257, 5, 64, 1000, 6, 4096), (6000, 255, 1000, 9, 256, 33), (7, 257, 65, 33, 4097, 64), (256, 9, 1000, 5, 257),
          (65, 255, 6, 7, 64), (5, 33, 255, 9), (), (6, 7, 65, 256))
C_PACKED = 8


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def shape_tables(t, um=UM, select=None, out_c=None):
    """One launch of ``demia_contour_shape`` over the tables: [M, out_c, 10] float64; rows the kernel did not write hold ``OUT_FILL``.
    Asserts that nothing was written behind the last row and that the tables it reads are unchanged."""
    import torch

    from deepemia_amd import _lib

    lib = _lib.load()
    dev = t.count.device
    out_c = t.C if out_c is None else int(out_c)
    sel = None
    if select is not None:
        flags = np.zeros(t.M, dtype=np.int32)
        flags[np.asarray(list(select), dtype=np.int64)] = 1
        sel = torch.from_numpy(flags).to(dev)
    wi = torch.empty((int(lib.demia_contour_shape_work_ints(t.M, t.C, t.max_points)),), dtype=torch.int32, device=dev)
    flat = torch.full((t.M * out_c * COLS + OUT_GUARD,), OUT_FILL, dtype=torch.float64, device=dev)
    out = flat[: t.M * out_c * COLS].view(t.M, out_c, COLS)
    before = t.points.clone()
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.demia_contour_shape(_lib.ptr(sel), _lib.ptr(t.count), _lib.ptr(t.info), _lib.ptr(t.red), _lib.ptr(t.points),
                                           t.M, t.C, t.max_points, _lib.ptr(wi), float(um), _lib.ptr(out), out_c, stream), "demia_contour_shape")
        host = flat.cpu().numpy()
    assert torch.equal(before, t.points) and np.array_equal(t.info.cpu().numpy(), t.host_info) and np.array_equal(t.red.cpu().numpy(), t.host_red)
    assert (host[t.M * out_c * COLS:] == OUT_FILL).all(), "demia_contour_shape wrote behind its output"
    return host[: t.M * out_c * COLS].reshape(t.M, out_c, COLS)


@pytest.fixture(scope="module")
def cases():
    """name -> Case: generated (n = 5 .. 6000), degenerate, traced (in place and at the offset (16000, 15000)), the spur."""
    out = CC.generated_cases() + CC.degenerate_cases() + CC.traced_cases() + [CC.Case("spur", SR.spur_contour())]
    assert len({c.name for c in out}) == len(out) == 36 + 6 + 16 + 1
    return {c.name: c for c in out}


@pytest.fixture(scope="module")
def layout(cases):
    """mask -> list of case names: the generated cases as ``PACKED`` lays them out, then degenerate, traced and spur contours."""
    free = {}
    for c in CC.generated_cases():
        free.setdefault(c.n, []).append(c.name)
    masks = [[free[n].pop(0) for n in row] for row in PACKED]
    assert not any(free.values())
    one, two, tri, rect, col, same = (c.name for c in CC.degenerate_cases())
    masks += [[one, two, tri, "spur"], [rect, col, same]]
    traced = [c.name for c in CC.traced_cases()]
    masks += [traced[:8], traced[8:]]
    assert sorted(n for ks in masks for n in ks) == sorted(cases)
    return masks


@pytest.fixture(scope="module")
def alone(gpu_device, cases):
    """Every contour in a launch of its own (M = 1, C = 1, off = 0): (values, area, perimeter)."""
    out = {}
    for name, c in cases.items():
        t = CC.tables_from_points([[c.points]], 1, gpu_device)
        out[name] = (shape_tables(t)[0, 0].copy(), float(t.host_red[0, 0, 0]), float(t.host_red[0, 0, 1]))
    return out


@pytest.fixture(scope="module")
def packed(gpu_device, cases, layout):
    t = CC.tables_from_points([[cases[n].points for n in ks] for ks in layout], C_PACKED, gpu_device)
    return t, shape_tables(t)


# ------------------------------------------------------------------------------------------------------ 1. values vs reference
def test_values_vs_reference(cases, alone):
    bad = []
    worst = 0.0
    for name, c in cases.items():
        got, area, per = alone[name]
        want = SR.shape_values(c.points, area, per, UM)
        for msg in SR.compare(got, want):
            bad.append((name, c.n, msg))
        for j in range(3, 9):
            if want[j]:
                worst = max(worst, abs(got[j] - want[j]) / abs(want[j]))
    print(f"kernel against the exact reference, {len(cases)} contours: worst relative difference of values 3..8 {worst:.3g} (bound {SR.REL_TOL:.3g})")
    assert not bad, bad


def test_degenerate_values(alone):
    assert (alone["one_point"][0] == np.array([0, 0, 1, 0, 0, 0, 0, 0, 0, 0.0])).all()
    assert (alone["identical5"][0] == np.array([0, 0, 1, 0, 0, 0, 0, 0, 0, 0.0])).all()
    v = alone["two_horizontal"][0]
    assert v[0] == 0 and v[1] == 8100 and v[2] == 2 and v[4] == 180 * UM and v[5] == 0 and v[7] == 90 * UM and v[8] == 0 and v[9] == 0
    v = alone["collinear6"][0]
    assert v[0] == 0 and v[1] == 2450 and v[2] == 2 and v[8] == 0 and abs(v[9] - 135.0) <= SR.ANGLE_TOL
    v = alone["rectangle"][0]                                           # 9 x 19: two tied diagonals, the tie rule fixes the angle
    assert v[0] == 2 * 9 * 19 and v[1] == 81 + 361 and v[2] == 4 and v[5] == 1.0
    assert abs(v[9] - (180.0 - np.degrees(np.arctan2(19, 9)))) <= SR.ANGLE_TOL
    assert alone["spur"][0][2] == 5 and alone["spur"][0][0] == 209 and alone["spur"][0][1] == 180


# -------------------------------------------------------------------------------------------------------- 2. layout invariance
def test_layout_invariance_bit_for_bit(gpu_device, cases, layout, alone, packed):
    t, vals = packed

    def same(got, m, c, name, what):
        assert (_bits(got[m, c]) == _bits(alone[name][0])).all(), (what, name, m, c, got[m, c], alone[name][0])

    for m, ks in enumerate(layout):                                     # several contours per mask, contours c >= 4 among them
        for c, name in enumerate(ks):
            same(vals, m, c, name, "packed")
        assert (vals[m, len(ks):] == OUT_FILL).all(), m                # slots without a contour stay untouched
    # the masks in reverse order, another C, the pool laid out in another order with room in front and between
    rev = layout[::-1]
    n_c = sum(len(ks) for ks in rev)
    t2 = CC.tables_from_points([[cases[n].points for n in ks] for ks in rev], 9, gpu_device,
                               pool_order=list(np.random.default_rng(8).permutation(n_c)), gap=3, lead=5)
    assert not np.array_equal(np.sort(t2.host_info[..., 3].ravel()), np.sort(t.host_info[..., 3].ravel()))
    v2 = shape_tables(t2)
    for m, ks in enumerate(rev):
        for c, name in enumerate(ks):
            same(v2, m, c, name, "reversed")
        assert (v2[m, len(ks):] == OUT_FILL).all(), m
    # select: every second mask; the others keep their fill
    sel = list(range(0, len(layout), 2))
    v3 = shape_tables(t, select=sel)
    for m, ks in enumerate(layout):
        if m in sel:
            for c, name in enumerate(ks):
                same(v3, m, c, name, "select")
            assert (v3[m, len(ks):] == OUT_FILL).all()
        else:
            assert (v3[m] == OUT_FILL).all(), m
    # fewer output slots than contours: the first two of every mask, nothing else
    v4 = shape_tables(t, out_c=2)
    assert v4.shape == (len(layout), 2, COLS) and min(len(ks) for ks in layout if ks) > 2
    for m, ks in enumerate(layout):
        for c, name in enumerate(ks[:2]):
            same(v4, m, c, name, "out_c=2")
        if not ks:
            assert (v4[m] == OUT_FILL).all()


# ---------------------------------------------------------------------------------------------------- 3. slots vs on demand
def _many_contours_mask():
    h, w = 200, 224
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((h, w), bool)
    m[5:25, 5:15] = True
    m[((xx - 70) * 0.6 - (yy - 65) * 0.8) ** 2 / 38 ** 2 + ((xx - 70) * 0.8 + (yy - 65) * 0.6) ** 2 / 22 ** 2 <= 1] = True
    m[((xx - 160) * 0.8 + (yy - 50) * 0.6) ** 2 / 40 ** 2 + (-(xx - 160) * 0.6 + (yy - 50) * 0.8) ** 2 / 15 ** 2 <= 1] = True
    m[120:180, 10:30] = True
    m[150:170, 50:150] = True
    m[190:195, 200:220] = True
    m[110, 200] = True
    return m


def test_launch_shape_slots_equals_shape(gpu_device):
    """``launch("shape", slots=4)`` + ``fetch`` against ``descriptor("shape")``: a set whose masks fit the slots (the values ride on the fetch) and a
    mask with more contours than slots (the fallback computes them on demand)."""
    from deepemia_amd.maskset import MaskOps

    ops = MaskOps(gpu_device)
    many = _many_contours_mask()
    few = np.zeros_like(many)
    few[30:90, 40:100] = True
    few[60, 100:120] = True                                             # a spur: repeated points
    few[150:160, 20:200] = True
    for masks, fallback in ((np.stack([many, np.zeros_like(many)]), True), (np.stack([few, np.zeros_like(few), few[::-1].copy()]), False)):
        planes = ops.from_dense(masks)
        cs = ops.trace(planes, max_contours=16)
        cs.launch_measure(UM, slots=4)
        cs.launch("shape", UM, slots=4)
        cs.fetch(with_points=True)
        st = cs.launched["shape"]
        first = st.dev.cpu().numpy()                                    # [M, 4, 10]
        assert (st.host is None) == fallback
        full = cs.descriptor("shape", UM)
        # on demand, on the SAME tables (a second trace may leave a mask's contours in other slots): as if nothing had ridden along
        carried, st.host = st.host, None
        demand = cs.descriptor("shape", UM)
        st.host = carried
        n = int(cs.host()[0].max())
        assert (n > 4) == fallback and full.shape == demand.shape == (len(masks), n, COLS)
        assert (_bits(full) == _bits(demand)).all()
        assert (_bits(first[:, :min(n, 4)]) == _bits(full[:, :4])).all()
        count = cs.host()[0]
        for m in range(len(masks)):
            assert not full[m, int(count[m]):].any()                   # rows as allocated
        recs = cs.records(um_pix=UM, descriptors=("shape",))
        plain = cs.records(um_pix=UM)
        assert all("shape" not in r for rs in plain for r in rs)
        for rs, ps in zip(recs, plain):
            assert len(rs) == len(ps)
            for r, p in zip(rs, ps):
                assert (_bits(r["values"]) == _bits(p["values"])).all()
                bad = SR.compare(r["shape"], SR.shape_values(r["points"], r["area"], r["perimeter"], UM))
                assert not bad, (r["points"].tolist()[:6], bad)


# ------------------------------------------------------------------------------------------------ 4. the 12 values untouched
def test_measure_values_are_untouched_by_a_shape_launch(packed):
    t, _ = packed
    before = CC.measure_tables(t)
    shape_tables(t)
    after = CC.measure_tables(t)
    assert (_bits(before) == _bits(after)).all()


# ------------------------------------------------------------------------------------------------------------------- 5. CLI
def test_cli_appends_seven_columns_in_every_mask_frame(tmp_path, monkeypatch, gpu_device):
    import main as cli
    from deepemia_amd import maskset
    from deepemia_amd.functions import inference as inf_mod
    from deepemia_amd.utils import config as C
    from test_gpu_cropset import DATASET, _set_frame, _write_tree

    ds_cfg = {"inference_overrides": {"confidence_mode": "manual",
                                      "class_specific_settings": {"class_0": {"confidence_threshold": 0.3, "iou_threshold": 0.6},
                                                                  "class_1": {"confidence_threshold": 0.35, "iou_threshold": 0.5}},
                                      "tile_settings": {"tile_size": 200, "overlap_ratio": 0.125, "upscale_factor": 1.0, "edge_filter_enabled": True},
                                      "spatial_constraints": {"enabled": True, "containment_rules": {1: 0}, "containment_threshold": 0.5}}}
    cfgdir, split = _write_tree(tmp_path, ds_cfg)
    monkeypatch.setenv("DEEPEMIA_CONFIG_DIR", str(cfgdir))
    monkeypatch.setenv("DEEPEMIA_OFFLINE", "1")
    monkeypatch.setenv("DEEPEMIA_WORKERS", "1")
    monkeypatch.chdir(tmp_path)

    # what the rows were made of: the records of ContourSet.records (with the um_pix they were asked at) and the rows of each call
    um_of, keep, checked = {}, [], []
    records = maskset.ContourSet.records
    rows_fn = inf_mod.measurement_rows

    def records_spy(self, um_pix=1.0, *a, **k):
        recs = records(self, um_pix, *a, **k)
        keep.append(recs)
        for rs in recs:
            for r in rs:
                um_of[id(r)] = um_pix
        return recs

    def rows_spy(image_name, classes, recs, thing_classes, min_area, *a, **k):
        rows = rows_fn(image_name, classes, recs, thing_classes, min_area, *a, **k)
        passing = [c for contours in recs for c in contours if not c["area"] < min_area]
        assert len(passing) == len(rows)
        checked.extend(zip(rows, passing))
        return rows

    monkeypatch.setattr(maskset.ContourSet, "records", records_spy)
    monkeypatch.setattr(inf_mod, "measurement_rows", rows_spy)

    names = ["measurements_results.csv", "R50_flip_results.csv"]
    outs = {}
    for frame, on in (("full", False), ("full", True), ("crop", True), ("crop_direct", True)):
        cfg = {"inference_overrides": dict(ds_cfg["inference_overrides"], **({"shape_descriptors": True} if on else {}))}
        _set_frame(cfgdir, cfg, frame)
        C.reset_cache()
        del checked[:]
        assert cli.main(["--task", "inference", "--dataset_name", DATASET, "--threshold", "0.3", "--no-gpu-check"]) == 0
        C.reset_cache()
        outs[frame, on] = {nm: (split / nm).read_bytes() for nm in names}
        for nm in names:
            (split / nm).unlink()
        if not on:
            assert all(len(row) == 20 and "shape" not in c for row, c in checked)
            continue
        # every row of this run: its seven new fields against the reference on the contour's own points ...
        assert len(checked) > 10
        for row, c in checked:
            assert len(row) == 27
            want = SR.shape_values(c["points"], c["area"], c["perimeter"], um_of[id(c)])
            assert (_bits(np.array(row[20:], dtype=np.float64)) == _bits(c["shape"][3:])).all()      # (values 0..2 are not in the file)
            bad = SR.compare(c["shape"], want)
            assert not bad, (row[0], bad)
        # ... and those rows are the file's rows
        buf = io.StringIO()
        w = csv.writer(buf)
        for row, _ in checked:
            w.writerow(row)
        lines = outs[frame, on]["measurements_results.csv"].decode().splitlines()
        assert sorted(buf.getvalue().splitlines()) == sorted(lines[1:])

    off = outs["full", False]
    off_rows = list(csv.reader(io.StringIO(off["measurements_results.csv"].decode(), newline="")))
    assert len(off_rows) > 10 and all(len(r) == 20 for r in off_rows)
    for frame in ("full", "crop", "crop_direct"):
        got = outs[frame, True]
        assert got == outs["full", True], frame                                             # both files, byte for byte, in every frame
        assert got["R50_flip_results.csv"] == off["R50_flip_results.csv"]
    on_text = outs["full", True]["measurements_results.csv"].decode()
    on_rows = list(csv.reader(io.StringIO(on_text, newline="")))
    assert on_rows[0] == inf_mod.CSV_HEADER + inf_mod.SHAPE_CSV_HEADER and len(on_rows[0]) == 27
    assert all(len(r) == 27 for r in on_rows) and len(on_rows) == len(off_rows)
    # the first 20 fields of every line are the bytes of the run with the setting off
    off_lines = off["measurements_results.csv"].decode().split("\r\n")
    on_lines = on_text.split("\r\n")
    assert len(on_lines) == len(off_lines)
    for a, b in zip(on_lines, off_lines):
        assert a[:len(b)] == b and (a == b == "" or a[len(b)] == ","), (a, b)
