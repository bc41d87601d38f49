"""The ROI pooler's reference and case table, checked without a GPU.

  * every named case of ``roi_align_cases.py`` reaches the branch it is named for, by the reference's own diagnostics;
  * the reference (``roi_align_ref.py``: direct per-sample form, f32 geometry, f64 sums) agrees with the oracle
    (``oracle.maskrcnn_ref.roi_pool``: vectorised torch f32, another summation order) on the whole table -- which is also
    the MEASUREMENT the GPU tolerance is derived from: the largest ``|oracle - reference| / amax(level features)`` is
    printed, and must stay by the record of it, ``roi_align_cases.ORACLE_VS_REF``.
"""
import numpy as np
import pytest
import torch

import roi_align_cases as T
import roi_align_ref as REF


@pytest.fixture(scope="module")
def diags():
    """The reference's decisions for every case at every pool size."""
    return {P: [REF.box_diag(b, P, T.SIZES) for b in T.BOXES] for P in T.POOL_SIZES}


def _kept(axis):
    return [v for s in axis["coords"] for v in s]


def test_every_named_case_reaches_its_branch(diags):
    bad = []
    for i, c in enumerate(T.CASES):
        e = c.expect
        d = diags[e["P"]][i]
        y, x = d["y"], d["x"]
        got = {"level": d["level"], "gy": y["g"], "gx": x["g"], "skipped_y": y["skipped"], "skipped_x": x["skipped"]}
        for k in ("level", "gy", "gx", "skipped_y", "skipped_x"):
            if k in e and got[k] != e[k]:
                bad.append((c.name, k, got[k], e[k]))
        for k, axis in (("has_y", y), ("has_x", x)):
            if k in e and e[k] not in _kept(axis):
                bad.append((c.name, k, _kept(axis)))
        if e.get("all_skipped") and not (y["skipped"] == e["P"] * y["g"] and x["skipped"] == e["P"] * x["g"] and y["g"] > 0 and x["g"] > 0):
            bad.append((c.name, "all_skipped", y["skipped"], x["skipped"]))
        for b, n in e.get("touched_x", {}).items():
            if x["touched"][b] != n:
                bad.append((c.name, "touched_x", b, x["touched"][b]))
        if "nine" in e:
            axis, b = e["nine"]
            if d[axis]["touched"][b] != 9 or d[axis]["g"] != 7:
                bad.append((c.name, "nine", d[axis]["g"], d[axis]["touched"]))
    assert not bad, bad


def test_the_exact_edge_samples_are_kept_and_the_next_float_is_not():
    """-1 and ``size`` themselves pass the strict tests; one f32 step further out does not."""
    f32 = np.float32
    for size in (40, 128):
        for v, kept in ((f32(-1.0), True), (np.nextafter(f32(-1.0), f32(-2.0)), False), (f32(size), True), (np.nextafter(f32(size), f32(1e9)), False)):
            # a box whose single sample (P = 1, g = 1) lies on v: start = v - 0.5, extent 1 (scale 1: c = start + 0.5)
            g, bins = REF.axis_samples(f32(v), f32(v) + f32(1.0), 1.0, 1, size)
            assert g == 1 and bins[0][0][0] == v and bins[0][0][1] == kept, (size, v, bins)


def test_no_other_case_touches_more_than_g_plus_1_pixels(diags):
    """The nine-pixel bins are the named ones and nothing else (so a failure of another case is not this defect), and no
    bin of the separable path's range touches more than nine."""
    nine = {(i, c.expect["P"], c.expect["nine"][0]) for i, c in enumerate(T.CASES) if "nine" in c.expect}
    assert len(nine) >= 10
    seen = set()
    for P in T.POOL_SIZES:
        for i, d in enumerate(diags[P]):
            for axis in ("y", "x"):
                g, most = d[axis]["g"], max(d[axis]["touched"])
                if g > 7:
                    continue
                assert most <= g + 2, (T.NAMES[i], P, axis, g, most)
                if most > g + 1:
                    seen.add((i, P, axis))
    assert seen == nine, (seen ^ nine)


def test_levels_of_the_table_cover_the_pyramid_and_both_paths(diags):
    levels = [d["level"] for d in diags[7]]
    assert set(levels) == {0, 1, 2, 3}
    for P, least in ((7, 6), (14, 2)):
        fallback = sum(1 for d in diags[P] if d["y"]["g"] > 7 or d["x"]["g"] > 7)
        tables = sum(1 for d in diags[P] if 1 <= d["y"]["g"] <= 7 and 1 <= d["x"]["g"] <= 7)
        assert tables >= 20 and fallback >= least, (P, tables, fallback)


def test_reference_on_a_constant_map_is_the_kept_fraction():
    """Bilinear weights sum to 1: on an all-ones pyramid a bin's value is (kept samples) / (gh gw), exactly what the
    diagnostics count -- ties the values to the decisions without any other implementation."""
    ones = [np.ones((h, w, 1), dtype=np.float32) for (h, w) in T.SIZES]
    for name in ("over_left_edge_by_a_third", "sample_just_past_minus_1_y", "wholly_outside", "zero_width", "empty_left_bin_live_right_bin",
                 "nine_rows_P7_bin0", "fallback_gh15", "bulk_00", "bulk_17"):
        box = T.BOXES[T.NAMES.index(name)]
        out, d = REF.roi_align_box(ones, box, 7)
        gy, gx = d["y"]["g"], d["x"]["g"]
        # kept samples per bin = g - skipped in that bin: recount from the coordinates
        H, W = T.SIZES[d["level"]]
        ky = [sum(1 for v in s if -1.0 <= v <= H) for s in d["y"]["coords"]]
        kx = [sum(1 for v in s if -1.0 <= v <= W) for s in d["x"]["coords"]]
        want = np.outer(ky, kx) / float(max(gy * gx, 1))
        np.testing.assert_allclose(out[..., 0], want, rtol=0, atol=1e-6, err_msg=name)     # (l + h is 1 to an f32 rounding)


def test_reference_agrees_with_the_oracle_on_the_whole_table():
    from oracle import maskrcnn_ref as R

    feats = T.features()
    levels = [np.moveaxis(f, 0, 2) for f in feats]                     # [H, W, N, C]: both images in one reference pass
    amax = np.stack([np.abs(f).reshape(T.N_IMAGES, -1).max(axis=1) for f in feats])       # [level, image]
    boxes_t = torch.from_numpy(T.BOXES)
    worst = (0.0, None)
    for P in T.POOL_SIZES:
        ref, dg = REF.roi_pool(levels, T.BOXES, P)                     # [R, P, P, N, C]
        lv = np.array([d["level"] for d in dg])
        assert (R.assign_levels(boxes_t).numpy() == lv).all()
        for n in range(T.N_IMAGES):
            pyr = [torch.from_numpy(f[n]).permute(2, 0, 1)[None].contiguous() for f in feats]
            got = R.roi_pool(pyr, boxes_t, P).permute(0, 2, 3, 1).numpy().astype(np.float64)
            err = np.abs(got - ref[:, :, :, n]).reshape(T.R, -1).max(axis=1) / amax[lv, n]
            i = int(err.argmax())
            if err[i] > worst[0]:
                worst = (float(err[i]), (T.NAMES[i], P, n))
    print(f"largest |oracle - reference| / amax(level): {worst[0]:.3e} at {worst[1]}")
    # (the oracle's f32 sums are torch reductions, whose order may differ a little from one CPU to the next: half as much again)
    assert worst[0] <= 1.5 * T.ORACLE_VS_REF, worst
    assert worst[0] >= T.ORACLE_VS_REF / 4, ("the record is stale: measure again", worst)
