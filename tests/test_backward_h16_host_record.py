"""The host side of the five codebook backward units on bf16 / fp16 activations against a record of what it did before their MFMA
plan and their glue were written once: every *_h16 plan and workspace query over the half sweep of
tools/backward_host_record.py, and the return code and nnc_last_error() text of every invalid call, equal
tests/golden/backward_h16_host_record.json.  That record was made by the same tool from a library built at the commit before the
refactor, never from the library under test.  The invalid calls fail before any HIP call, so none of this needs a device."""
import importlib.util
import json
import os

import pytest

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tool():
    spec = importlib.util.spec_from_file_location("backward_host_record", os.path.join(ROOT, "tools", "backward_host_record.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib(tool):
    nbuild.build_native()
    return tool.bind(nat.lib_path())


@pytest.fixture(scope="module")
def record():
    with open(os.path.join(ROOT, "tests", "golden", "backward_h16_host_record.json")) as f:
        return json.load(f)


def test_the_sweep_is_the_one_the_record_was_made_over(tool, record):
    """ten half plan and ten half workspace entry points, every m of the sweep, both dtypes, every call counted"""
    names = {k.split("|")[0] for k in record["plans"]}
    assert len(names) == 20 and all(n.endswith(("_h16_plan", "_h16_workspace_bytes")) for n in names)
    assert {k.split("|m=")[1] for k in record["plans"]} == {str(m) for m in tool.M}
    assert len(record["plans"]) == 20 * len(tool.M)
    shapes = len(tool.KDIM) * len(tool.NCOLS)
    assert record["plans"]["nnc_cbmm_dx_h16_plan|m=1"][0] == shapes * len(tool.BYTE_LK) * len(tool.DTYPES) * len(tool.CUS) * len(tool.ADDR)
    assert record["plans"]["nnc_cbsp_dc_h16_plan|m=128"][0] == shapes * len(tool.BYTE_LK) * len(tool.DTYPES) * len(tool.CUS)
    assert record["plans"]["nnc_cbpk_grouped_dc_h16_plan|m=17"][0] == shapes * len(tool.PACKED_BK) * len(tool.GROUP_ROWS) * len(tool.DTYPES) * len(tool.CUS)
    assert record["plans"]["nnc_cbmm_grouped_dc_h16_workspace_bytes|m=256"][0] == shapes * len(tool.GROUPED_K) * len(tool.GROUP_ROWS)
    called = {r[0] for r in record["invalid"]}
    assert len(called) == 30 and {n for n in called if n.endswith("_h16")} == {f"{f}_{d}_h16" for f in tool.FORMS for d in ("dx", "dc")}
    # every entry point is refused on a stream and on an MFMA shape, for each of the things only the half calls check
    for f in tool.FORMS:
        for d, changed in (("dx", ("dt", "dxdt", "g", "dx", "ws")), ("dc", ("dt", "x", "g", "dc", "ws"))):
            for m in tool.HALF_M_INVALID:
                seen = {k for r in record["invalid"] if r[0] == f"{f}_{d}_h16" and r[1].get("m") == m for k in r[1]}
                assert set(changed) <= seen, (f, d, m)
    assert all(r[2] != 0 for r in record["invalid"] if r[0].endswith(("_h16", "_plan")))


def test_every_plan_and_workspace_query_answers_as_before(tool, lib, record):
    got = tool.sweep_plans(lib, half=True)
    assert set(got) == set(record["plans"])
    wrong = [k for k in sorted(got) if got[k] != record["plans"][k]]
    assert not wrong, wrong


def test_every_invalid_call_fails_with_the_same_code_and_text(tool, lib, record):
    got = json.loads(json.dumps(tool.sweep_invalid(lib, half=True)))
    assert len(got) == len(record["invalid"])
    wrong = [(g, w) for g, w in zip(got, record["invalid"]) if g != w]
    assert not wrong, wrong[:5]
