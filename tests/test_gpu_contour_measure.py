"""GPU: the twelve values per contour of ``contour_measure_kernel`` (``csrc/contours.hip``), fed with plain tables built from
integer point lists (``tests/contour_cases.py``), so that the sizes are chosen and not whatever a tracer produces.

References: the independent float64 geometry of ``contour_cases.py`` (scipy hull + every edge's rectangle, set-valued over the
int truncation; ``numpy.linalg`` conic fit; closed forms) with the ellipse bounds fixed by ``test_cpu_contour_geometry.py``
on the CPU, and -- separately, so that a failure tells which of the two moved -- the oracle at 1e-7.

Kernel branches the case table reaches: ``in_lds`` on (n <= 256, including 255 / 256) and off (257 ... 6000, several of them
at once out of the shared work pools); rank sort (n <= 4096, including 4096) and lane-0 heapsort (4097, 6000); one row per
lane and wrap-around in the wave's least squares (64 / 65); the first ellipse fit (n = 5) and none (n < 5); hulls of 1, 2 and
more points; contours c >= MEAS_CG = 4 of one mask, LDS-sized and HBM-sized ones alternating in one block's loop; ``select``
with skipped masks; ``out_c < count[m]``; an empty mask; frame coordinates up to 16500.

Seen on an MI355X (printed by the first test, asserted against the CPU-derived bounds only): worst relative ellipse difference
to the float64 reference 1.53e-6 for n < 10 and 8.96e-8 for n >= 10 -- the oracle's own figures to the digit.
"""
import numpy as np
import pytest

import contour_cases as CC

pytestmark = pytest.mark.gpu

# The packed launch: contour sizes per mask (the k-th use of a size takes its k-th repetition).  36 cases, one empty mask,
# five masks with contours c >= MEAS_CG = 4.  Blocks (m, c % 4) walk slots c and c + 4: mask 0 has HBM-sized -> LDS-sized
# (257 -> 6) and LDS-sized -> HBM-sized with the heapsort (5 -> 4096), mask 1 a full LDS after the largest contour
# (6000 -> 256), mask 3 the two sides of the LDS boundary in one loop (256 -> 257).  All nine HBM-sized contours share one grid.
PACKED = ((257, 5, 64, 1000, 6, 4096), (6000, 255, 1000, 9, 256, 33), (7, 257, 65, 33, 4097, 64), (256, 9, 1000, 5, 257),
          (65, 255, 6, 7, 64), (5, 33, 255, 9), (), (6, 7, 65, 256))
C_PACKED = 8


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def layout():
    """mask -> list of indices into the generated cases."""
    cases = CC.generated_cases()
    free = {}
    for k, c in enumerate(cases):
        free.setdefault(c.n, []).append(k)
    masks = [[free[n].pop(0) for n in row] for row in PACKED]
    assert not any(free.values()) and sum(len(ks) for ks in masks) == len(cases) == 36
    return masks


@pytest.fixture(scope="module")
def packed(gpu_device, layout):
    cases = CC.generated_cases()
    t = CC.tables_from_points([[cases[k].points for k in ks] for ks in layout], C_PACKED, gpu_device)
    return t, CC.measure_tables(t)


@pytest.fixture(scope="module")
def alone(gpu_device):
    """Every generated and every degenerate contour measured by a launch of its own: M = 1, C = 1, off = 0."""
    out = {}
    for c in CC.generated_cases() + CC.degenerate_cases():
        t = CC.tables_from_points([[c.points]], 1, gpu_device)
        assert t.host_info[0, 0, 3] == 0
        out[c.name] = CC.measure_tables(t)[0, 0].copy()
    return out


def test_values_vs_independent_reference(packed, layout):
    t, vals = packed
    cases = CC.generated_cases()
    bad = []
    worst = {True: 0.0, False: 0.0}                                      # relative ellipse difference, keyed by n < 10
    for m, ks in enumerate(layout):
        for c, k in enumerate(ks):
            area, per = t.host_red[m, c]
            for msg in CC.check_against_reference(vals[m, c], cases[k].points, float(area), float(per)):
                bad.append((cases[k].name, m, c, msg))
            for j, e in enumerate(CC.ref_ellipse(cases[k].points)):
                worst[cases[k].n < 10] = max(worst[cases[k].n < 10], abs(vals[m, c, j] - e) / abs(e))
        assert (vals[m, len(ks):] == CC.OUT_FILL).all(), m             # slots without a contour stay untouched
    print(f"kernel against the float64 reference, worst relative ellipse difference: n < 10 {worst[True]:.3g} "
          f"(bound {CC.ELLIPSE_BOUND_SMALL_N:.3g}), n >= 10 {worst[False]:.3g} (bound {CC.ELLIPSE_BOUND:.3g})")
    assert not bad, bad


def test_values_vs_oracle(packed, layout):
    t, vals = packed
    cases = CC.generated_cases()
    bad = []
    for m, ks in enumerate(layout):
        for c, k in enumerate(ks):
            exp, unstable = CC.oracle_values(cases[k].points)
            for j, key in enumerate(CC.KEYS):
                if unstable and j < 3:
                    continue
                if not abs(vals[m, c, j] - exp[j]) <= 1e-7 * max(1.0, abs(exp[j])):
                    bad.append((cases[k].name, key, vals[m, c, j], exp[j]))
    assert not bad, bad


def test_layout_invariance_bit_for_bit(gpu_device, packed, layout, alone):
    cases = CC.generated_cases()
    t, vals = packed

    def same(got, m, c, k, what):
        assert (_bits(got[m, c]) == _bits(alone[cases[k].name])).all(), (what, cases[k].name, m, c, got[m, c], alone[cases[k].name])

    for m, ks in enumerate(layout):
        for c, k in enumerate(ks):
            same(vals, m, c, k, "packed")
    # the masks in reverse order, another C, the pool laid out in another order with room in front and between
    rev = layout[::-1]
    n_c = sum(len(ks) for ks in rev)
    t2 = CC.tables_from_points([[cases[k].points for k in ks] for ks in rev], 6, gpu_device,
                               pool_order=list(np.random.default_rng(8).permutation(n_c)), gap=3, lead=5)
    assert not np.array_equal(np.sort(t2.host_info[..., 3].ravel()), np.sort(t.host_info[..., 3].ravel()))
    v2 = CC.measure_tables(t2)
    for m, ks in enumerate(rev):
        for c, k in enumerate(ks):
            same(v2, m, c, k, "reversed")
    # select: every second mask; the others keep their fill
    sel = list(range(0, len(layout), 2))
    v3 = CC.measure_tables(t, select=sel)
    for m, ks in enumerate(layout):
        if m in sel:
            for c, k in enumerate(ks):
                same(v3, m, c, k, "select")
            assert (v3[m, len(ks):] == CC.OUT_FILL).all()
        else:
            assert (v3[m] == CC.OUT_FILL).all(), m
    # fewer output slots than contours: the first two of every mask, nothing else
    v4 = CC.measure_tables(t, out_c=2)
    assert v4.shape == (len(layout), 2, 12) and min(len(ks) for ks in layout if ks) > 2
    for m, ks in enumerate(layout):
        for c, k in enumerate(ks[:2]):
            same(v4, m, c, k, "out_c=2")
        if not ks:
            assert (v4[m] == CC.OUT_FILL).all()


def test_launch_measure_slots_equals_measure(gpu_device):
    """``ContourSet.launch_measure(slots=4)`` + ``fetch()`` against ``measure()`` on a traced mask with more contours than slots."""
    from deepemia_amd.maskset import MaskOps
    from oracle import postproc_ref as P

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
    masks = np.stack([m, np.zeros_like(m)])
    ops = MaskOps(gpu_device)
    cs = ops.trace(ops.from_dense(masks), max_contours=16)
    cs.launch_measure(CC.UM, slots=4)
    cs.fetch()
    first = cs._vals_dev.cpu().numpy()                                   # [2, 4, 12]
    full = cs.measure(CC.UM)
    n = int(cs.host()[0][0])
    assert n >= 6 and full.shape[1] == n and int(cs.host()[0][1]) == 0
    assert (_bits(first[0]) == _bits(full[0, :4])).all()
    assert not first[1].any() and not full[1].any()                     # the empty mask: rows as allocated
    recs = cs.records(um_pix=CC.UM)[0]
    ref = P.find_external_contours(m)
    assert len(recs) == len(ref) == n
    for rec, c in zip(recs, ref):
        np.testing.assert_array_equal(rec["points"], c)
        if len(np.unique(c, axis=0)) >= 3 and len(c) != 3:
            bad = CC.check_against_reference(rec["values"], c, rec["area"], rec["perimeter"])
            assert not bad, (c.tolist()[:6], bad)


def test_degenerate_contours(gpu_device, alone):
    um = CC.UM
    one, two, tri, rect, col, same = CC.degenerate_cases()
    groups = [[one, two, tri], [], [rect, col, same]]
    t = CC.tables_from_points([[c.points for c in g] for g in groups], 4, gpu_device)
    vals = CC.measure_tables(t)
    assert (vals[1] == CC.OUT_FILL).all()                                # the empty mask between the others
    got = {}
    for m, g in enumerate(groups):
        assert (vals[m, len(g):] == CC.OUT_FILL).all()
        for c, case in enumerate(g):
            got[case.name] = vals[m, c]
            assert (_bits(vals[m, c]) == _bits(alone[case.name])).all(), (case.name, vals[m, c], alone[case.name])
            area, per = t.host_red[m, c]
            bad = CC.check_against_reference(vals[m, c], case.points, float(area), float(per), ellipse=False,
                                             ties="all" if case.n == 3 else "raise")
            assert not bad, (case.name, bad)
    assert not got["one_point"].any()
    v = got["two_horizontal"]
    assert v[3] == 0 and abs(v[4] - 90 * um) <= CC.RECT_TOL * um and v[6] == 0 and v[10] == 0 and not v[:3].any()
    assert abs(v[9] - 90 * um) <= CC.RECT_TOL * um and v[8] == 180 * um and v[5] == 0
    for name in ("triangle", "rectangle"):
        assert not got[name][:3].any()
    v = got["rectangle"]
    assert abs(v[3] - 9 * um) <= CC.RECT_TOL * um and abs(v[4] - 19 * um) <= CC.RECT_TOL * um
    length, width = CC.two_point_closed_form((2000, 40), (2035, 75))
    v = got["collinear6"]
    # the hn == 2 rectangle has zero height; its ends are integers, which the f32 corner arithmetic may miss by a rounding
    assert (v[3], v[4]) in [(pytest.approx(l, abs=CC.RECT_TOL * um), pytest.approx(w_, abs=CC.RECT_TOL * um))
                            for l, w_ in CC.rect_candidates(col.points)]
    assert abs(v[4] - width) <= 1.5 * um and v[3] <= 1.5 * um and length == 0
    v = got["identical5"]
    assert not v[3:].any()
    for name in ("collinear6", "identical5"):                            # the oracle flags these fits unstable: any value,
        assert all(np.isfinite(x) or np.isnan(x) for x in got[name][:3])   # finite or NaN, but the same in every launch
