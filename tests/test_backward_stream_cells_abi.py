"""CPU checks of the stream-cell case list of the backward units (tests/helpers/stream_cells_ref.py): at 80, 256
and 304 CUs the dx and dc plans of every unit put every case into the cell it is built for, with the column blocks, splits and row
groups it claims; between them the cases reach every entry of the hard-coded tables; and the tables equal the lists of instantiations
in the sources, read as text, so an instantiation added without a case turns this file red.  No device needed."""
import os
import re

import pytest

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from tests.helpers import stream_cells_ref as cells

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "neural_network_compression_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_the_case_counts():
    """one case per cell x m x width (x the two ways to be unaligned): 8 values of m over the five mt"""
    assert sum(len(v) for v in cells.MS_OF_MT.values()) == 8
    assert len(cells.CASES["byte"]) == 2 * 8 * 2 * 3 and len(cells.CASES["grouped"]) == 8 * 2 * 3 and len(cells.CASES["sparse"]) == 2 * 8 * 2
    for form, cases in cells.CASES.items():
        assert len({c["id"] for c in cases}) == len(cases)
        assert {cells.cell_of(c) for c in cases} == cells.CELLS[form]
    assert len(cells.BYTE_CELLS) == 20 and len(cells.SPARSE_CELLS) == 10 and len(cells.GROUPED_CELLS) == 10


@pytest.mark.parametrize("unit", sorted(cells.UNITS))
def test_every_case_lands_in_its_cell_and_every_cell_is_hit(lib, unit):
    form, dtypes, _ = cells.UNITS[unit]
    for dtype in dtypes:
        for cus in cells.CU_COUNTS:
            hit = {"dx": set(), "dc": set()}
            for case in cells.CASES[form]:
                dx, dc, dx_ws, dc_ws = cells.plans(case, dtype, cus)
                for which, p in (("dx", dx), ("dc", dc)):
                    what = (unit, dtype, cus, case["id"], which, p)
                    assert p["path"] == cells.PATH_STREAM, what
                    assert cells.cell_of_plan(case, p) == cells.cell_of(case), what
                    assert p["mt"] >= case["m"] > p["mt"] // 2, what
                    for field, want in case["expect"][which].items():
                        assert p[field] == want, (what, field)
                    if form == "sparse":
                        assert p["segs"] == case["segs"], what
                    hit[which].add(cells.cell_of_plan(case, p))
                assert dx["workspace"] == dx_ws and dc["workspace"] == dc_ws
                G = -(-case["kdim"] // case["group_rows"]) if form == "grouped" else 1
                assert dc_ws == 64 + 8 * G * case["k"]
                if form == "sparse":       # the partials, rounded up to 256 bytes, then the row sums of g
                    part = dx["splits"] * case["m"] * case["kdim"] * 4 if dx["splits"] > 1 else 0
                    assert dx_ws == (part + 255) // 256 * 256 + 4 * case["m"]
                else:
                    assert dx_ws == (dx["splits"] * case["m"] * case["kdim"] * 4 if dx["splits"] > 1 else 0)
            assert hit["dx"] == hit["dc"] == cells.CELLS[form], (unit, dtype, cus)


def _source(name):
    return open(os.path.join(CSRC, name)).read()


def _macro_list(text, name):
    """[(vb, mt)] of ``#define NAME(X) X(vb, mt) ...``"""
    (body,) = re.findall(r"#define " + name + r"\(X\)(.*)", text)
    got = [(int(a), int(b)) for a, b in re.findall(r"X\((\d+),\s*(\d+)\)", body)]
    assert re.sub(r"X\(\d+,\s*\d+\)", "", body).strip() == "", body
    return got


def test_the_tables_are_the_lists_in_the_sources():
    hpp = _source("nnc_cbgrad.hpp")
    u8, u16 = _macro_list(hpp, "CBG_U8_STREAM_CASES"), _macro_list(hpp, "CBG_U16_STREAM_CASES")
    assert [(1, vb, mt) for vb, mt in u8] + [(2, vb, mt) for vb, mt in u16] == list(cells.BYTE_TABLE)
    assert u8 == list(cells.GROUPED_TABLE)
    # which lists each unit's table is made of
    uses = {name: re.findall(r"CBG_(U8|U16)_STREAM_CASES\(", _source(name)) for name in
            ("nnc_cbgrad.hip", "nnc_cbgrad_h16.hip", "nnc_cbgrad_grouped.hip", "nnc_cbgrad_grouped_h16.hip")}
    assert uses == {"nnc_cbgrad.hip": ["U8", "U16"], "nnc_cbgrad_h16.hip": ["U8", "U16"] * 2, "nnc_cbgrad_grouped.hip": ["U8"],
                    "nnc_cbgrad_grouped_h16.hip": ["U8"] * 2}
    sg = re.findall(r"SG_CASE\(uint(\d+)_t,\s*(\d+),\s*(\d+)\)", _source("nnc_cbspgrad.hip"))
    sgh = re.findall(r"SGH_CASE\(XT,\s*uint(\d+)_t,\s*(\d+),\s*(\d+)\)", _source("nnc_cbspgrad_h16.hip"))
    for got in (sg, sgh):
        assert all(int(bits) == 8 * int(lb) for bits, lb, _ in got)
        assert [(int(lb), int(mt)) for _, lb, mt in got] == list(cells.SPARSE_TABLE)
    assert re.findall(r"SGH_CASES\((\w+)\)\}", _source("nnc_cbspgrad_h16.hip")) == ["bf16_t", "f16_t"]
    assert {src for _, _, src in cells.UNITS.values()} == set(uses) | {"nnc_cbspgrad.hip", "nnc_cbspgrad_h16.hip"}


def test_the_exactness_precondition_holds_for_every_case():
    """data() asserts it; the largest sum of magnitudes over all cases, in quarters, stays below 1.7e6 (2^24 is 16.8e6)"""
    top = 0.0
    for form, cases in cells.CASES.items():
        for case in cases:
            for dtype in cells.DTYPES:
                d = cells.data(case, dtype)
                assert d["dx"].shape == (case["m"], case["kdim"])
                assert d["dc"].shape == ((3, case["k"]) if form == "grouped" else (case["k"],))
                top = max(top, d["top"])
    assert 4.0 * top < 1.7e6, top
