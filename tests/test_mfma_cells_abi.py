"""CPU checks of the MFMA-cell case lists of the fifteen half-precision codebook units (tests/helpers/mfma_cells_ref.py, DESIGN.md
section 34): the table of instantiations of every unit equals its kMfmaCases list (or dispatch) and its hm_launch / dcm_xvec call
site, read from the sources as text, and the arm rule equals the text of hm_launch and dcm_xvec; at 80, 256 and 304 CUs the plan of
every unit puts every case on the MFMA path with the tiles, splits, per_split and groups it claims, and the addresses and widths put
it into the arm it claims; between them the cases reach all 208 cells, every elem cell by width and by address, every cell with every
edge value; the exactness precondition holds for every case.  No device needed."""
import os
import re

import numpy as np
import pytest

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from tests.helpers import cbgrad_ref, grouped_h16_grad_ref
from tests.helpers import mfma_cells_ref as cells

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "neural_network_compression_amd", "csrc")
XT = {"bf16": "bf16_t", "fp16": "f16_t"}


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def _source(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_counts():
    assert [sum(len(t) for (f, d), t in cells.TABLES.items() if d == way) for way in cells.DIRECTIONS] == [32, 36, 36]
    assert sum(len(c) for c in cells.CELLS.values()) == 208
    assert cells.SPLIT_EXTENT == {"vec": 136, "elem": 141} and cells.DIRECT_EXTENT == {"vec": 56, "elem": 61}
    n = {unit: len(cases) for unit, cases in cells.CASES.items()}
    # per argument: plain forms 2 + 2 slots a mode (dc: 2 + 8), grouped forms 6 + 6
    assert n == {("byte", "fwd"): 16, ("sparse", "fwd"): 16, ("gbyte", "fwd"): 24, ("gpacked", "fwd"): 48, ("gsparse", "fwd"): 24,
                 ("byte", "dx"): 16, ("sparse", "dx"): 16, ("packed", "dx"): 16, ("gbyte", "dx"): 24, ("gpacked", "dx"): 48,
                 ("byte", "dc"): 40, ("sparse", "dc"): 40, ("packed", "dc"): 40, ("gbyte", "dc"): 24, ("gpacked", "dc"): 48}
    assert sum(n.values()) == 440


# ------------------------------------------------------------------ the tables against the sources
def _arg_name(form, a):
    if a is None:
        return None
    return f"uint{8 * a}_t" if form in ("byte", "sparse") else str(a)


@pytest.mark.parametrize("unit", sorted(cells.UNITS), ids=lambda u: "-".join(u))
def test_the_table_is_the_list_in_the_source(unit):
    """every launch_*mfma<...> the source names outside the template's own definition is a table entry and the reverse; the kernel is
    instantiated exactly twice, as the two arms of one hm_launch / dcm_xvec call over the operands the arm rule names"""
    form, way = unit
    src_name, kernel, args = cells.UNITS[unit]
    src = _source(src_name)
    launch = {"fwd": "launch_mfma", "dx": "launch_dx_mfma", "dc": "launch_dc_mfma"}[way]
    used = re.findall(launch + r"<(\w+)(?:, (\w+))?>", src)
    want = sorted((XT[dt], _arg_name(form, a) or "") for dt in cells.DTYPES for a in args)
    assert sorted(used) == want, (unit, used)
    assert {(dt, a) for dt, a, _ in cells.TABLES[unit]} == {(dt, a) for dt in cells.DTYPES for a in args}
    if "kMfmaCases" in src:         # the list holds one entry per (element type, argument), each naming its own launch
        (body,) = re.findall(r"static const MfmaCase kMfmaCases\[\] = \{(.*?)\};", src, flags=re.S)
        entries = re.findall(r"\{NNC_DT_(BF16|F16)(?:, (\d))?, ([^{}]*)\}", body)
        assert len(entries) == 2 * len(args), (unit, entries)
        for dt, a, fns in entries:
            x = {"BF16": "bf16_t", "F16": "f16_t"}[dt]
            lt = {"": "", "0": ""}.get(a, f", uint{8 * int(a or 1)}_t" if form in ("byte", "sparse") else f", {a}")
            assert f"{launch}<{x}{lt}>" in fns, (unit, dt, a, fns)
    else:                           # nnc_cbmm_grouped.hip, nnc_cbpk_grouped.hip: a conditional over the element type (and the bits)
        assert form in ("gbyte", "gpacked") and way == "fwd"
        assert len(re.findall(r"x_dtype == NNC_DT_BF16 \? \(?(?:bits == 4 \? )?launch_mfma<bf16_t", src)) == 1
    targs = {"byte": "<XT, LT, {}>", "sparse": "<XT, LT, {}>", "packed": "<XT, BITS, {}>", "gpacked": "<XT, BITS, {}>", "gbyte": "<XT, {}>", "gsparse": "<XT, {}>"}[form]
    vec, elem = kernel + targs.format("true"), kernel + targs.format("false")
    if way == "dc":
        assert f"dcm_xvec(x, g, kdim, ncols) ? {vec} : {elem})" in src
    else:
        assert f"hm_launch({'x, kdim' if way == 'fwd' else 'g, ncols'}, {vec}, {elem}, grid, lds, s, reinterpret_cast<const XT *>({'x' if way == 'fwd' else 'g'})" in src
    assert len(re.findall(re.escape(kernel) + "<", src)) == 2, unit                     # no third instantiation
    assert len(re.findall(r"void " + re.escape(kernel) + r"\(", src)) == 1


def test_the_arm_rule_is_the_launch_code():
    hm = _source("nnc_cbmfma.hpp")
    assert "const bool xvec = reinterpret_cast<uintptr_t>(x) % 16 == 0 && kdim % 8 == 0;" in hm
    assert "hipLaunchKernelGGL(xvec ? vec : elem, grid, dim3(HM_THREADS), lds, s, args...);" in hm
    assert ("return reinterpret_cast<uintptr_t>(x) % 4 == 0 && reinterpret_cast<uintptr_t>(g) % 4 == 0 && kdim % 2 == 0 && ncols % 2 == 0;"
            in _source("nnc_cbgrad_h16.hpp"))
    for way, (xa, ga, kdim, ncols), arm in (("fwd", (256, 2, 56, 33), "vec"), ("fwd", (258, 0, 56, 33), "elem"), ("fwd", (256, 0, 60, 33), "elem"),
                                            ("dx", (2, 256, 33, 56), "vec"), ("dx", (0, 264, 33, 56), "elem"), ("dx", (0, 256, 33, 60), "elem"),
                                            ("dc", (260, 264, 34, 194), "vec"), ("dc", (258, 256, 34, 194), "elem"), ("dc", (256, 258, 34, 194), "elem"),
                                            ("dc", (256, 256, 33, 194), "elem"), ("dc", (256, 256, 34, 193), "elem")):
        assert cells.arm_of(way, xa, ga, kdim, ncols) == arm
    plan = _source("nnc_cbh16plan.hpp")
    assert "std::min({cdiv(2LL * CB_PLAN_CUS, tiles), extent / (2 * HM_BK), 16LL})" in plan and "per_split = cdiv(cdiv(extent, s), HM_BK) * HM_BK;" in plan
    mm = _source("nnc_cbmm.hpp")
    assert "#define HM_BM 128" in mm and "#define HM_BN 128" in mm and "#define HM_BK 32" in mm and "#define CB_PLAN_CUS 256" in mm


# ------------------------------------------------------------------ the cases against the plans
@pytest.mark.parametrize("unit", sorted(cells.UNITS), ids=lambda u: "-".join(u))
def test_every_case_lands_in_its_cell_and_every_cell_is_hit(lib, unit):
    form, way = unit
    for cus in cells.CU_COUNTS:
        hit = set()
        for case in cells.CASES[unit]:
            xa, ga = cells.operand_addrs(case)
            assert cells.arm_of(way, xa, ga, case["kdim"], case["ncols"]) == case["arm"], case["id"]
            assert (case["how"] == "vec") == (case["arm"] == "vec") and (case["xoff"] + case["goff"] == 1) == case["how"].startswith("address")
            if case["how"].startswith("address"):      # a vec-eligible shape: at offset 0 it is the other arm
                assert cells.arm_of(way, 256, 256, case["kdim"], case["ncols"]) == "vec", case["id"]
            for dtype in cells.DTYPES:
                p, ws = cells.plan(case, dtype, cus)
                splits, per = cells.check_plan(case, p, cus)
                assert (splits > 1) == (case["mode"] == "split")
                out_units = {"fwd": case["m"] * case["ncols"], "dx": case["m"] * case["kdim"]}.get(way)
                if way != "dc":
                    assert p["workspace"] == ws == (splits * out_units * 4 if splits > 1 else 0), (case["id"], cus, p, ws)
                else:
                    assert p["workspace"] == ws and ws % 8 == 0, (case["id"], cus, p, ws)
                if form == "gpacked" and way == "fwd":
                    q, ws1 = cells.plan(case, dtype, cus, one_group=True)
                    assert cells.check_plan(case, q, cus, one_group=True) == (splits, per) and ws1 == ws
                hit.add((dtype, case["arg"], case["arm"], case["mode"]))
        assert hit == cells.CELLS[unit], (unit, cus, cells.CELLS[unit] - hit)


def test_every_cell_sees_every_edge():
    """per cell: both row values and both column values of the output tiles; an elem cell by width and by address (dc: by either width
    and either address); both epilogue values; a grouped cell every group_rows, a last group shorter than 32 rows, and 4, 2 and 1
    tables / sets of bins in a tile (dx, dc) or a second split that opens inside a group (forward, split)"""
    for unit, cases in cells.CASES.items():
        form, way = unit
        for a in cells.UNITS[unit][2]:
            for arm in cells.ARMS:
                for mode in cells.MODES:
                    mine = [c for c in cases if (c["arg"], c["arm"], c["mode"]) == (a, arm, mode)]
                    what = (unit, a, arm, mode)
                    rows = {c["kdim"] if way == "dc" else c["m"] for c in mine}
                    cols = {c["ncols"] if way != "dx" else c["kdim"] for c in mine}
                    assert {cells.cdiv(r, 128) for r in rows} == {cells.cdiv(c, 128) for c in cols} == {1, 2}, what
                    if way != "dc":
                        assert (rows, cols) == ({17, 161}, {33, 193}), what
                    elif arm == "vec":
                        assert rows == cols == {34, 194}, what
                    else:       # by width the odd value itself (kdim: rows, ncols: columns), by address the even one
                        assert rows == cols == {33, 34, 193, 194}, what
                        assert {c["kdim"] for c in mine if c["how"] == "width-k"} == {c["ncols"] for c in mine if c["how"] == "width-n"} == {33, 193}, what
                    if arm == "elem":
                        assert {c["how"] for c in mine} == set(cells.ELEM_HOWS[way]), what
                    if way == "fwd":
                        assert {c["bias"] for c in mine} == {c["relu"] for c in mine} == {True, False}, what
                    if way == "dc":
                        assert {c["m"] for c in mine} == set(cells.EXTENT[mode].values()), what
                    if form in ("byte", "gbyte") and a in (1, None):
                        assert sum(c["nan_centre"] for c in mine) == 1, what
                    if form in ("packed", "gpacked"):
                        assert {c["k"] for c in mine} == {1 << a, cells.SMALL_K[a]}, what
                    if form in cells.GROUPED:
                        assert {c["group_rows"] for c in mine} == {32, 64, 96, 128, cells.BIG_GROUP}, what
                        assert any(c["kdim"] > c["group_rows"] and 0 < c["kdim"] % c["group_rows"] < 32 for c in mine), what
                        assert any(c["groups"] == 1 for c in mine), what
                        if way == "fwd" and mode == "split":
                            inside = [c for c in mine if all(cells.second_split_opens_inside_a_group(c, cus) for cus in cells.CU_COUNTS)]
                            assert inside and all(c["group_rows"] in (64, 128) for c in inside), what
                        if way != "fwd":
                            assert {cells.tile_tables(c) for c in mine} == {1, 2, 4}, what
                            assert {grouped_h16_grad_ref.tile_tables(c["group_rows"]) for c in mine} == {1, 2, 4}, what
                            assert any(c["group_rows"] == 96 and cells.tile_tables(c) == 2 for c in mine), what      # the boundary off the tile grid


# ------------------------------------------------------------------ the older lists, counted
# unit -> (cells the older list reaches, of how many); the argument-arm-mode triples it misses (with both element types each)
BEFORE = {
    ("byte", "fwd"): (8, 16, {(1, "vec", "direct"), (1, "vec", "split"), (2, "vec", "direct"), (2, "vec", "split")}),
    ("sparse", "fwd"): (8, 16, {(1, "vec", "direct"), (1, "vec", "split"), (2, "vec", "direct"), (2, "vec", "split")}),
    ("gbyte", "fwd"): (6, 8, {(None, "vec", "direct")}),
    ("gpacked", "fwd"): (12, 16, {(2, "vec", "direct"), (4, "vec", "direct")}),
    ("gsparse", "fwd"): (6, 8, {(None, "vec", "direct")}),
    ("byte", "dx"): (10, 16, {(1, "vec", "direct"), (2, "vec", "direct"), (2, "vec", "split")}),
    ("sparse", "dx"): (14, 16, {(1, "vec", "direct")}),
    ("packed", "dx"): (10, 16, {(2, "vec", "direct"), (2, "vec", "split"), (4, "vec", "direct")}),
    ("gbyte", "dx"): (6, 8, {(None, "vec", "direct")}),
    ("gpacked", "dx"): (12, 16, {(2, "vec", "direct"), (4, "vec", "direct")}),
    ("byte", "dc"): (8, 16, {(1, "elem", "direct"), (1, "vec", "split"), (2, "elem", "direct"), (2, "vec", "split")}),
    ("sparse", "dc"): (10, 16, {(1, "vec", "split"), (2, "vec", "direct"), (2, "vec", "split")}),
    ("packed", "dc"): (8, 16, {(2, "elem", "direct"), (2, "vec", "split"), (4, "elem", "direct"), (4, "vec", "split")}),
    ("gbyte", "dc"): (8, 8, set()),
    ("gpacked", "dc"): (12, 16, {(2, "elem", "split"), (4, "elem", "direct")}),
}


def test_the_cells_the_older_lists_reach(lib):
    """the before column of DESIGN.md section 34: every older hand-picked list run through its unit's plan call and the arm rule (x and g
    at the start of a 256-byte aligned allocation, a buf[1:] view one element in), the same at 80, 256 and 304 CUs: 138 of 208 cells"""
    old = cells.old_lists()
    assert set(old) == set(cells.UNITS) == set(BEFORE)
    total = 0
    for unit, (_, plan_fn, rows) in old.items():
        hits = [cells.cells_reached(unit, plan_fn, rows, cus) for cus in cells.CU_COUNTS]
        assert hits[0] == hits[1] == hits[2], unit
        reached, of, missed = BEFORE[unit]
        assert (len(hits[0]), len(cells.CELLS[unit])) == (reached, of), unit
        assert cells.CELLS[unit] - hits[0] == {(dt,) + c for dt in cells.DTYPES for c in missed}, unit
        total += reached
    assert total == 138


# ------------------------------------------------------------------ the data
def test_the_exactness_precondition_holds_for_every_case():
    """data() asserts it per case from the float64 reference alone (four times the largest sum of magnitudes, bias included, below
    2^24); here every case is built: the largest sum stays below 6.5e3, and a ReLU case has both signs"""
    top = 0.0
    for unit, cases in cells.CASES.items():
        form, way = unit
        for case in cases:
            d = cells.data(case)
            if way == "fwd":
                assert d["y"].shape == (case["m"], case["ncols"]) and (d["bias"] is not None) == case["bias"]
                if case["relu"]:
                    assert (d["y"] == 0).any() and (d["y"] > 0).any() and not (d["y"] < 0).any()
            else:
                assert d["dx"].shape == (case["m"], case["kdim"])
                assert d["dc"].shape == ((case["groups"], case["k"]) if form in cells.GROUPED else (case["k"],))
            if case["oob"]:
                assert (d["labels"] >= case["k"]).any()
            if case["nan_centre"]:
                assert np.isnan(np.asarray(d["centers"]).reshape(-1, 256)[:, 255]).all() and np.isnan(d["centers"]).sum() == case.get("groups", 1)
            top = max(top, d["top"])
    assert 4.0 * top < 2.0 ** 15, top


def test_the_formulas_are_the_references_of_the_byte_form():
    """dx and dc of the generic reference equal cbgrad_ref.dx64 / dc64 on the byte cases (a NaN centre is used by no label)"""
    for way in ("dx", "dc"):
        for case in cells.CASES[("byte", way)][::3]:
            d = cells.data(case)
            cen = np.where(np.isnan(d["centers"]), 0.0, d["centers"]).astype(np.float32)
            assert np.array_equal(d["dx"], cbgrad_ref.dx64(d["g"], d["labels"], cen)), case["id"]
            assert np.array_equal(d["dc"], cbgrad_ref.dc64(d["x"], d["g"], d["labels"], case["k"])), case["id"]
