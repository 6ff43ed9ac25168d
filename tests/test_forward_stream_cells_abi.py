"""CPU checks of the stream-cell case lists of the forward units and of the packed half backward
(tests/helpers/forward_stream_cells_ref.py): at 80, 256 and 304 CUs the plan of every unit puts every case into
the cell it is built for, on the stream path, with the column blocks, splits and groups it claims; between them the cases reach every
entry of the hard-coded tables, each in both modes; and the tables equal the lists of instantiations in the sources, read as text, so
a case removed from a list or an instantiation added without a case turns this file red.  No device needed."""
import os
import re

import numpy as np
import pytest

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from tests.helpers import forward_stream_cells_ref as cells
from tests.helpers import packed_ref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "neural_network_compression_amd", "csrc")
FORWARD_UNITS = sorted(u for u, (form, _, _) in cells.UNITS.items() if not form.endswith("_bwd"))
BACKWARD_UNITS = sorted(u for u, (form, _, _) in cells.UNITS.items() if form.endswith("_bwd"))


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_the_case_counts():
    """8 values of m over the five mt; per cell and m: three kdim (two direct, one split) x two widths (x the three alignments of the
    byte forms); a wide packed cell has one direct and one split shape"""
    n = cells.CASES
    assert len(n["byte"]) == 2 * 8 * 3 * 2 * 3 and len(n["grouped"]) == 8 * 3 * 2 * 3 and len(n["sparse"]) == 2 * 8 * 3 * 2
    wide = sum(len(cells.MS_OF_MT[mt]) for _, _, mt in cells.WIDE)
    narrow = sum(len(cells.MS_OF_MT[mt]) for cell in cells.PACKED_TABLE if cell not in cells.WIDE for mt in cell[2:])
    assert (wide, narrow) == (9, 16) and len(n["packed"]) == len(n["gpacked"]) == 2 * wide + 6 * narrow
    assert len(n["packed_bwd"]) == len(n["gpacked_bwd"]) == wide + 2 * narrow
    for form, cases in n.items():
        assert len({c["id"] for c in cases}) == len(cases)
        assert {c["cell"] for c in cases} == cells.CELLS[form]
    assert [len(cells.CELLS[f]) for f in ("byte", "sparse", "grouped", "packed", "gpacked", "packed_bwd", "gpacked_bwd")] == [20, 10, 10, 18, 18, 18, 18]


def test_every_cell_sees_every_epilogue():
    """per cell: both modes, bias present and absent, ReLU on and off; with four cases or more a mode, each mode sees all of them"""
    for form in ("byte", "sparse", "grouped", "packed", "gpacked"):
        for cell in cells.CELLS[form]:
            mine = [c for c in cells.CASES[form] if c["cell"] == cell]
            assert {c["mode"] for c in mine} == {"direct", "split"}, (form, cell)
            assert {c["bias"] for c in mine} == {c["relu"] for c in mine} == {True, False}, (form, cell)
            if form in ("packed", "gpacked"):
                assert {c["oob"] for c in mine} == {True, False} or cell in cells.WIDE, (form, cell)
            for mode in ("direct", "split"):
                of_mode = [c for c in mine if c["mode"] == mode]
                if len(of_mode) >= 4:
                    assert {(c["bias"], c["relu"]) for c in of_mode} == {(a, b) for a in (True, False) for b in (True, False)}, (form, cell, mode)


def test_the_grouped_cases_walk_their_groups():
    """split: three groups or more, the last one short and, in the byte form, a boundary inside a split at every CU count; direct: one
    group (kdim 31) and two with a short last one (61)"""
    for form in ("grouped", "gpacked"):
        for c in cells.CASES[form]:
            groups, short = c["expect"]["groups"], c["kdim"] % c["group_rows"]
            if c["mode"] == "split":
                assert groups >= 3 and short, c["id"]
                if form == "grouped":
                    assert all(cells.groups_in_a_split(c, cus) >= 2 for cus in cells.CU_COUNTS), c["id"]
                else:
                    assert groups == 3, c["id"]
            else:
                assert (c["kdim"], groups) in ((31, 1), (61, 2)) and short, c["id"]


@pytest.mark.parametrize("unit", FORWARD_UNITS)
def test_every_case_lands_in_its_cell_and_every_cell_is_hit_in_both_modes(lib, unit):
    form, dtypes, _ = cells.UNITS[unit]
    for dtype in dtypes:
        for cus in cells.CU_COUNTS:
            hit = set()
            for case in cells.CASES[form]:
                p, ws = cells.plan(case, dtype, cus)
                hit.add((cells.check_plan(case, p, cus), case["mode"]))
                assert p["workspace"] == (p["splits"] * case["m"] * case["ncols"] * 4 if p["splits"] > 1 else 0) or form == "sparse"
                assert ws >= p["workspace"] and (ws == p["workspace"] or cus < cells.PLAN_CUS), (case["id"], cus, ws, p)   # (the query plans for 256 CUs)
                if form == "byte":          # aligned by the address too: the same call with the labels one byte on is unaligned
                    q, _ = cells.plan(case, dtype, cus, cells.labels_addr(case) + 1)
                    assert q["aligned"] == 0 and (q["vb"], q["mt"]) == (p["vb"], p["mt"])
                if form == "gpacked" and dtype != "f32":      # nnc_cbpk_h16: the same cell and splits with one group
                    q, _ = cells.plan(case, dtype, cus, one_group=True)
                    assert cells.check_plan(case, q, cus, one_group=True) == case["cell"]
            assert hit == {(cell, mode) for cell in cells.CELLS[form] for mode in ("direct", "split")}, (unit, dtype, cus)


@pytest.mark.parametrize("unit", BACKWARD_UNITS)
def test_every_packed_backward_case_lands_in_its_cell(lib, unit):
    form, dtypes, _ = cells.UNITS[unit]
    for dtype in dtypes:
        for cus in cells.CU_COUNTS:
            hit = {"dx": set(), "dc": set()}
            for case in cells.CASES[form]:
                dx, dc, dx_ws, dc_ws = cells.bwd_plans(case, dtype, cus)
                for which, p in (("dx", dx), ("dc", dc)):
                    what = (dtype, cus, case["id"], which, p)
                    assert p["path"] == cells.PATH_STREAM and cells.cell_of_plan(case, p) == case["cell"], what
                    assert p["mt"] >= case["m"] > p["mt"] // 2 and p["col_tiles"] == case["expect"]["col_tiles"], what
                    assert p["row_tiles"] >= 3, what
                    if form == "gpacked_bwd":
                        assert (p["group_rows"], p["groups"]) == (case["group_rows"], 3) and p["max_groups_per_workgroup"] >= 1, what
                    hit[which].add(cells.cell_of_plan(case, p))
                assert dx["splits"] == case["expect"]["splits"] and dc["splits"] == 1
                assert dx["workspace"] == dx_ws == (dx["splits"] * case["m"] * case["kdim"] * 4 if dx["splits"] > 1 else 0)
                assert dc["workspace"] == dc_ws
            assert hit["dx"] == hit["dc"] == cells.CELLS[form], (dtype, cus)


# ------------------------------------------------------------------ the tables against the sources
def _source(name):
    return open(os.path.join(CSRC, name)).read()


def _ints(found):
    return [tuple(int(v) for v in t) for t in found]


def _block(text, start, end):
    """the text from ``start`` up to the next ``end``"""
    (body,) = re.findall(re.escape(start) + r"(.*?)" + re.escape(end), text, flags=re.S)
    return body


def test_the_tables_are_the_lists_in_the_sources():
    T = cells.TABLES
    # byte form: float32 (kStreamCases, complete before this file) and bf16 / fp16
    body = _block(_source("nnc_cbmm.hip"), "static const StreamCase kStreamCases[] = {", "};")
    got = _ints(re.findall(r"\{(\d+), (\d+), (\d+), launch_stream<uint(\d+)_t, (\d+), (\d+)>\}", body))
    assert [(lb, vb, mt) for lb, vb, mt, _, _, _ in got] == list(T["byte"]) and all((8 * g[0], g[1], g[2]) == g[3:] for g in got)
    assert body.count("launch_stream") == len(T["byte"])
    h16 = _source("nnc_cbmm_h16.hip")
    body = _block(h16, "#define H16_STREAM_CASES(DT, XT)", "static const StreamCase")
    got = _ints(re.findall(r"\{DT, (\d+), (\d+), (\d+), launch_stream<XT, uint(\d+)_t, (\d+), (\d+)>\}", body))
    assert [(lb, vb, mt) for lb, vb, mt, _, _, _ in got] == list(T["byte"]) and all((8 * g[0], g[1], g[2]) == g[3:] for g in got)
    assert body.count("launch_stream") == len(T["byte"])
    assert re.findall(r"H16_STREAM_CASES\(NNC_DT_(\w+), (\w+)\)", h16) == [("BF16", "bf16_t"), ("F16", "f16_t")]
    # sparse form: float32 (complete before this file) and bf16 / fp16
    body = _block(_source("nnc_cbsp.hip"), "static const SpStreamCase kSpStreamCases[] = {", "};")
    got = _ints(re.findall(r"\{(\d+), (\d+), launch_sp_stream<uint(\d+)_t, (\d+)>\}", body))
    assert [(lb, mt) for lb, mt, _, _ in got] == list(T["sparse"]) and all((8 * g[0], g[1]) == g[2:] for g in got)
    assert body.count("launch_sp_stream") == len(T["sparse"])
    sph = _source("nnc_cbsp_h16.hip")
    body = _block(sph, "#define SP_H16_STREAM_CASES(DT, XT)", "static const StreamCase")
    got = _ints(re.findall(r"\{DT, (\d+), (\d+), launch_stream<XT, uint(\d+)_t, (\d+)>\}", body))
    assert [(lb, mt) for lb, mt, _, _ in got] == list(T["sparse"]) and all((8 * g[0], g[1]) == g[2:] for g in got)
    assert body.count("launch_stream") == len(T["sparse"])
    assert re.findall(r"SP_H16_STREAM_CASES\(NNC_DT_(\w+), (\w+)\)", sph) == [("BF16", "bf16_t"), ("F16", "f16_t")]
    # grouped byte form
    grp = _source("nnc_cbmm_grouped.hip")
    body = _block(grp, "#define GROUPED_STREAM_CASES(DT, XT)", "static const StreamCase")
    got = _ints(re.findall(r"\{DT, (\d+), (\d+), launch_stream<XT, (\d+), (\d+)>\}", body))
    assert [g[:2] for g in got] == list(T["grouped"]) and all(g[:2] == g[2:] for g in got) and body.count("launch_stream") == len(T["grouped"])
    assert re.findall(r"GROUPED_STREAM_CASES\(NNC_DT_(\w+), (\w+)\)", grp) == [("F32", "float"), ("BF16", "bf16_t"), ("F16", "f16_t")]
    # packed form and grouped packed form (nnc_cbpk_h16 calls the latter with one group)
    body = _block(_source("nnc_cbpk.hip"), "static const PkStreamCase kPkStreamCases[] = {", "};")
    assert _ints(re.findall(r"PK_CASE\((\d+), (\d+), (\d+)\)", body)) == list(T["packed"]) and body.count("PK_CASE") == len(T["packed"])
    pkg = _source("nnc_cbpk_grouped.hip")
    body = _block(pkg, "#define PKG_STREAM_CASES(DT, XT)", "static const StreamCase")
    assert _ints(re.findall(r"PKG_CASE\(DT, XT, (\d+), (\d+), (\d+)\)", body)) == list(T["packed"]) and body.count("PKG_CASE") == len(T["packed"])
    assert re.findall(r"PKG_STREAM_CASES\(NNC_DT_(\w+), (\w+)\)", pkg) == [("F32", "float"), ("BF16", "bf16_t"), ("F16", "f16_t")]
    assert "nnc_cbpk_grouped(" in _block(_source("nnc_cbpk_h16.hip"), 'extern "C" int nnc_cbpk_h16(', "\n}")
    # the packed backward list, and the units that are made of it
    body = _block(_source("nnc_cbpkgrad.hpp"), "#define PKG_STREAM_CASES(X)", "\n\n")
    assert sorted(_ints(re.findall(r"X\((\d+), (\d+), (\d+)\)", body))) == sorted(T["packed"]) and body.count("X(") == len(T["packed"])
    assert re.findall(r"PKG_STREAM_CASES\((\w+)\)", _source("nnc_cbpk_h16.hip")) == ["BF_CASE", "HF_CASE"]
    assert re.findall(r"PKG_STREAM_CASES\((\w+)\)", _source("nnc_cbpkgrad_grouped_h16.hip")) == ["BF_CASE", "HF_CASE"]
    # grouped sparse form, forward (complete before this file) and backward
    body = _block(_source("nnc_cbsp_grouped.hpp"), "#define SPG_STREAM_CASES(DT, XT)", "\n\n")
    got = _ints(re.findall(r"\{DT, (\d+), launch_spg_stream<XT, (\d+)>\}", body))
    assert [a for a, _ in got] == list(T["gsparse"]) and all(a == b for a, b in got) and body.count("launch_spg_stream") == len(T["gsparse"])
    (sgg,) = re.findall(r"static const SggCase kSggCases\[\] = \{(.*?)\};", _source("nnc_cbspgrad_grouped.hip"))
    assert [int(v) for v in re.findall(r"SGG_CASE\((\d+)\)", sgg)] == list(T["gsparse"]) and sgg.count("SGG_CASE") == len(T["gsparse"])
    assert {src for _, _, src in cells.UNITS.values()} == {"nnc_cbmm_h16.hip", "nnc_cbsp_h16.hip", "nnc_cbmm_grouped.hip", "nnc_cbpk.hip",
                                                           "nnc_cbpk_grouped.hip", "nnc_cbpk_h16.hip", "nnc_cbpkgrad_grouped_h16.hip"}


# ------------------------------------------------------------------ the data
def test_the_fast_pack_is_the_reference_pack():
    rng = np.random.RandomState(3)
    for bits, kdim, ncols in ((4, 5, 33), (2, 3, 65), (4, 2, 32), (2, 7, 1)):
        lab = rng.randint(0, 1 << bits, size=(kdim, ncols)).astype(np.uint8)
        assert np.array_equal(cells.pack(lab, bits), packed_ref.pack(lab, kdim, ncols, bits))


def test_the_exactness_precondition_holds_for_every_narrow_case():
    """data() asserts it for every case it builds, the wide packed shapes included (the GPU file builds those); here every other case
    is built: the largest sum of magnitudes, in quarters, stays below 2.1e6 (2^24 is 16.8e6), and a ReLU case has both signs"""
    top = 0.0
    for unit in FORWARD_UNITS:
        form, dtypes, _ = cells.UNITS[unit]
        for case in cells.CASES[form]:
            if case.get("wide"):
                continue
            for dtype in dtypes:
                d = cells.data(case, dtype)
                assert d["y"].shape == (case["m"], case["ncols"]) and (d["bias"] is not None) == case["bias"]
                if case["relu"]:
                    assert (d["y"] == 0).any() and (d["y"] > 0).any() and not (d["y"] < 0).any()
                top = max(top, d["top"])
    for form in ("packed_bwd", "gpacked_bwd"):
        for case in cells.CASES[form]:
            if not case["wide"]:
                d = cells.bwd_data(form, case["id"])
                assert d["dx"].shape == (case["m"], case["kdim"]) and d["dc"].shape == ((3, case["k"]) if form == "gpacked_bwd" else (case["k"],))
                top = max(top, d["top"])
    assert 4.0 * top < 2.1e6, top
