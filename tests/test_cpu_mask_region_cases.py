"""CPU: the case table of ``tests/mask_region_cases.py`` is what it says it is, and the reference can tell.

* every case lands in the variant, flood body and band relation its name claims, by the restated ``region_of`` / variant rule
  for the program it runs with;
* families A-G together reach every boundary, residue and edge the GPU test is there for (asserted as a list);
* the restated region stages (lockstep flood on runs, seeds, Euler shortcut) equal scipy on every case when left to converge --
  so the model is checked -- and each deliberately wrong flood differs from scipy on the cases of the family that targets it:
  if the kernel had that fault, ``test_gpu_mask_region_edges.py`` would fail;
* the lockstep model needs more rounds than ``2 * (rh + 32 * rw) + 8`` on every adversarial serpentine with 8 waves and fewer
  on the controls, and never more than the proven ``32 * rh * rw + 1``.

Lockstep rounds (rounds in which some word changes) beside the legacy limit, as computed here:
64 x 500: 1744 / 1164; 130 x 2040: 7643 / 4368; 20 x 2080: 6235 / 4276; control 30 x 250 (4 waves): 434 / 584; 64 x 500 with
horizontal legs: 7 / 1164.
"""
import numpy as np
import pytest

import mask_region_cases as M
from oracle import postproc_ref as P

_REF = {}


def ref(c):
    """(mask after the first stage, flag) from scipy, once per mask and stage."""
    key = (id(c.mask), c.program[0])
    if key not in _REF:
        _REF[key] = M.run_program_ref(c.mask, c.program[:1], None, P)
    return _REF[key]


def model(c, **kw):
    """What the restated region stages give for the case's FIRST stage: (mask, flag, rounds)."""
    g = M.geometry(c)
    box = g.get("box", M.EMPTY)
    e = g.get("e", 1)
    rm = M.RegionModel(**kw)
    if c.program[0] == "fill":
        out, rounds = rm.fill(c.mask, box, e)
        return out, 0, rounds
    multi, _, rounds = rm.multi(c.mask, box, e)
    return c.mask, int(multi), rounds


def agrees(c, **kw):
    m, f, _ = model(c, **kw)
    rm, rf = ref(c)
    return bool((m == rm).all()) and f == rf


def first_stage_cases(family):
    return [c for c in M.cases(family) if c.program[0] in ("fill", "flag_multi")]


def test_every_case_sits_where_its_name_says():
    n = 0
    for fam in M.FAMILIES:
        for c in M.cases(fam):
            g = M.geometry(c)
            if g["empty"]:
                assert not c.mask.any() and fam == "D", c.name               # the ring inside the border of a frame below 3 x 3
                continue
            for k, v in c.claim:
                if k == "path":
                    holes = bool((P.fill_holes(c.mask) != c.mask).any())
                    assert (v == "flood") == holes, c.name
                    assert M.RegionModel().multi(c.mask, g["box"])[1] == v, c.name
                else:
                    assert g[k] == v, (c.name, k, v, g[k])
            n += 1
    assert n > 700


def test_families_reach_every_boundary_residue_and_edge():
    geo = {fam: [(c, M.geometry(c)) for c in M.cases(fam)] for fam in "ABCDFG"}
    live = {fam: [(c, g) for c, g in v if not g["empty"]] for fam, v in geo.items()}
    # A: both sides of both variant boundaries, under both programs (the second margin changes n)
    for prog in M.A_PROGRAMS:
        got = sorted((g["n"], g["variant"]) for c, g in live["A"] if c.program == prog)
        assert got == [(1024, "small"), (1056, "large"), (8192, "large"), (8256, "hbm")], prog
    mixed, _ = M.mixed_batch()
    assert sorted(M.geometry(c).get("variant", "empty") for c in mixed) == ["empty", "hbm", "large", "small"]
    # B: every width of the chunked body in LDS and in HBM, region-relative chunk boundaries
    assert {(g["rw"], g["variant"]) for c, g in live["B"]} == {(rw, v) for rw in (65, 66, 129, 130) for v in ("large", "hbm")}
    assert all(g["body"] == "chunk" and g["wx0"] == 3 and (g["wx0"] + 64) % 64 != 0 for c, g in live["B"])
    assert all(g["body"] == "lane" for f in "ACDFG" for c, g in live[f] if g["rw"] <= 64) and any(g["rw"] == 64 for c, g in live["A"])
    # C: every row count with 4 waves, from 3 rows on with 8; fewer rows than waves, as many, one more; frames of 1 and 2 rows
    assert {g["rh"] for c, g in live["C"] if g["nw"] == 4} == set(M.C_ROWS)
    assert {g["rh"] for c, g in live["C"] if g["nw"] == 8} == {r for r in M.C_ROWS if r >= 3}
    for nw in (4, 8):
        rel = {np.sign(g["rh"] - nw) for c, g in live["C"] if g["nw"] == nw}
        assert rel == {-1, 0, 1}, nw
        assert any(g["bands"] < nw for c, g in live["C"] if g["nw"] == nw)                 # waves without a band
        assert any(g["rh"] % g["rpb"] for c, g in live["C"] if g["nw"] == nw)                 # a last band that is shorter
    assert {c.H for c, g in live["C"]} >= {1, 2} and {g["body"] for c, g in live["C"]} == {"lane", "chunk"}
    # D: widths around the word size, heights where first and last row coincide or touch, boxes clipped on every side
    assert {c.W % 32 for c, g in live["D"]} >= {0, 1, 31} and {c.W for c, g in live["D"]} == set(M.D_WIDTHS)
    assert {c.H for c, g in live["D"]} == set(M.D_HEIGHTS) and (1, 1) in {(c.H, c.W) for c, g in live["D"]}
    assert {k for c, g in live["D"] for k in range(4) if g["clipped"][k]} == {0, 1, 2, 3}
    assert all((g["wx0"] + g["rw"]) * 32 >= c.W for c, g in live["D"] if g["clipped"][3])     # the last, partial word is in the region
    assert any(g["empty"] for c, g in geo["D"])
    # E: the three hints move the same mask between regions and between variants
    moved = set()
    for fam in "ABCD":
        for c, g in live[fam]:
            vs = tuple(M.geometry(c, h)["variant"] for h in M.HINTS)
            moved.add(vs)
            assert M.geometry(c, "loose")["n"] >= g["n"] and M.geometry(c, "frame")["n"] >= M.geometry(c, "loose")["n"]
    assert {("small", "small", "hbm"), ("small", "large", "hbm"), ("large", "hbm", "hbm"), ("small", "small", "small")} <= moved, moved
    # F: eight slots, several dilations clipped at a frame corner, two flag stages, all three gates, stages after a drop
    progs = {(c.program, c.active) for c in M.cases("F")}
    assert any(len(p) == 8 and M.n_dilations(p) == 4 for p, _ in progs)
    assert {a for p, a in progs if p == ("gate", "dilate")} == {None, 0, 1}
    assert any(p.count("flag_multi") == 2 for p, _ in progs) and any(p[0] == "drop_multi" and len(p) > 1 for p, _ in progs)
    assert all(sum(g["clipped"]) >= 2 for c, g in live["F"])
    for c in M.cases("F"):
        if c.program == ("flag_multi", "dilate", "flag_multi") and "two_2px_apart" in c.name:
            out, flag = M.run_program_ref(c.mask, c.program, None, P)
            assert flag == 1 and P.n_components8(out) == 1                                  # the dilation joins them; the flag stays
        if c.program[0] == "drop_multi" and "two_2px_apart" in c.name:
            assert not M.run_program_ref(c.mask, c.program, None, P)[0].any()               # the later stages see an empty mask
        if c.program == ("gate", "dilate"):
            out, _ = M.run_program_ref(c.mask, c.program, c.active, P)
            assert bool((out == c.mask).all()) == (not c.active)
    # G: both ways of counting
    assert {dict(c.claim)["path"] for c in M.cases("G")} == {"euler", "flood"}


@pytest.mark.parametrize("family", ["A", "B", "C", "D", "G"])
def test_restated_stages_equal_scipy_when_left_to_converge(family):
    cs = first_stage_cases(family)
    assert cs
    for c in cs:
        assert agrees(c), c.name
        if family == "D" or not c.name.endswith("_fill"):
            continue
        assert agrees(M.with_hint(c, "frame")), c.name                                      # another region, the same answer


# fault of the restated flood -> (family that targets it, cases that must ALL notice, or None: at least one case)
FAULTS = {"chunk": ("B", "holes+channels"), "diag": ("B", "diag"), "bands": ("C", None), "seed": ("D", None), "margin": ("C", None)}


@pytest.mark.parametrize("wrong", sorted(FAULTS))
def test_reference_tells_each_wrong_flood_from_the_right_one(wrong):
    family, must = FAULTS[wrong]
    noticed = [c.name for c in first_stage_cases(family) if not agrees(c, wrong=wrong)]
    assert noticed, wrong
    if wrong == "chunk":
        want = [c.name for c in M.cases("B") if must in c.name and c.program == ("fill",)]
        want += [c.name for c in M.cases("B") if "diag" in c.name and c.program == ("flag_multi",)]
        assert set(want) <= set(noticed), sorted(set(want) - set(noticed))
    if wrong == "diag":
        want = [c.name for c in M.cases("B") if must in c.name and c.program == ("flag_multi",)]
        assert set(want) <= set(noticed), sorted(set(want) - set(noticed))
        assert all("_multi" in n for n in noticed)                                          # a 4-connected flood has no diagonal link
    if wrong == "bands":
        assert {M.geometry(c)["nw"] for c in M.cases("C") if c.name in noticed} == {4, 8}
    if wrong == "seed":
        # (with W % 32 != 0 the padding bits beyond W are seeds next to pixel W - 1, so only whole-word widths depend on this seed)
        assert {c.W for c in M.cases("D") if c.name in noticed} == {32, 64}


def test_lockstep_rounds_against_the_limits_on_the_serpentines():
    seen = {}
    for name, h, w, vert, x0, adversarial in M.H_SIZES:
        for c in M.cases("H"):
            if f"H_{name}_" not in c.name:
                continue
            g = M.geometry(c)
            legacy, proven = M.legacy_max_rounds(g["rh"], g["rw"]), M.proven_max_rounds(g["rh"], g["rw"])
            rm, rf = ref(c)
            assert (rm == c.mask).all() and rf == 0, c.name                                  # scipy: nothing to fill, one component
            m, f, rounds = model(c)
            assert (m == rm).all() and f == rf, c.name                                       # the model, left to converge, is scipy's flood
            assert rounds <= proven
            assert agrees(c, limit="proven"), c.name
            seen[c.name] = (rounds, legacy)
            if adversarial:
                assert g["nw"] == 8 and rounds > legacy, (c.name, rounds, legacy)
                # stopping there leaves the end of the channel to be filled as a hole; the walls all hang from the top row, so
                # the flood of the component from its first pixel is short and the component test comes out right either way
                assert agrees(c, limit="legacy") == (c.program == ("flag_multi",)), c.name
            else:
                assert rounds <= legacy, (c.name, rounds, legacy)
                assert agrees(c, limit="legacy"), c.name
            if "control" in name:
                assert g["nw"] == 4 and model(c, nw=8)[2] > legacy                           # the limit covers 4 waves, not 8
    assert seen["H_64x500_lds8_fill"] == (1744, 1164) and seen["H_30x250_control_fill"] == (434, 584), seen
