"""CPU checks of the group-wise codebook backward pass's C ABI (include/nnc.h, nnc_cbmm_grouped_dx_* / nnc_cbmm_grouped_dc_*;
DESIGN.md section 19): the symbols, the argument errors (returned before any HIP call, so none of this needs a device), the plans
against the ungrouped ones over CU counts, the regimes the shared case list claims, and the 2^62 bound of the integer sums."""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from neural_network_compression_amd import ops
from tests.helpers import grouped_grad_ref as ref

NNC_EINVAL, NNC_ENOSPACE = -1, -2
SYMBOLS = ("nnc_cbmm_grouped_dx_workspace_bytes", "nnc_cbmm_grouped_dx_plan", "nnc_cbmm_grouped_dx_f32",
           "nnc_cbmm_grouped_dc_workspace_bytes", "nnc_cbmm_grouped_dc_plan", "nnc_cbmm_grouped_dc_f32")
P = 0x1000   # a fake, never dereferenced address


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_symbols_are_declared_exported_and_bound(lib):
    """The six entry points are declared in include/nnc_cbgrad_grouped.h, which nnc.h includes, and bound from
    _native.GROUPED_GRAD_SIGNATURES: the text of nnc.h itself and _native.SIGNATURES are pinned by the older ABI tests."""
    raw = ctypes.CDLL(nat.lib_path())
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "nnc_cbgrad_grouped.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(nnc_[a-z0-9_]+)\s*\(", text)) == set(SYMBOLS) == set(nat.GROUPED_GRAD_SIGNATURES)
    assert '#include "nnc_cbgrad_grouped.h"' in open(os.path.join(inc, "nnc.h")).read()
    for s in SYMBOLS:
        assert hasattr(raw, s) and getattr(lib, s).argtypes == nat.GROUPED_GRAD_SIGNATURES[s][1]
    defs = {k: int(v) for k, v in re.findall(r"#define (NNC_\w+) (\d+)", text)}
    assert defs["NNC_CBGRAD_GROUPED_PLAN_LEN"] == nat.CBGRAD_GROUPED_PLAN_LEN
    for name in ("group_rows", "groups", "rows_per_group", "max_groups_per_workgroup"):
        assert defs["NNC_CBGRAD_GROUPED_P_" + name.upper()] == nat.CBDX_GROUPED_PLAN_FIELDS.index(name) == nat.CBDC_GROUPED_PLAN_FIELDS.index(name)
    assert nat.CBGRAD_GROUPED_PLAN_LEN == len(nat.CBDX_GROUPED_PLAN_FIELDS) == len(nat.CBDC_GROUPED_PLAN_FIELDS)


def dx_call(lib, g=P, m=4, kdim=64, labels=P, ncols=16, centers=P, k=16, group_rows=32, dx=P, ws=None, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbmm_grouped_dx_workspace_bytes(m, kdim, ncols) if min(m, kdim, ncols) >= 0 else 0
    return lib.nnc_cbmm_grouped_dx_f32(g, m, kdim, labels, ncols, centers, k, group_rows, dx, ws, ws_bytes, None)


def dc_call(lib, x=P, g=P, m=4, kdim=64, labels=P, ncols=16, k=16, group_rows=32, dc=P, f64=1, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ok = min(m, kdim, ncols) >= 0 and 1 <= k <= 256 and group_rows >= 32 and group_rows % 32 == 0
        ws_bytes = lib.nnc_cbmm_grouped_dc_workspace_bytes(m, kdim, ncols, k, group_rows) if ok else 0
    return lib.nnc_cbmm_grouped_dc_f32(x, g, m, kdim, labels, ncols, k, group_rows, dc, f64, ws, ws_bytes, None)


# cg_check's checks, the group_rows checks of nnc_cbmm_grouped, K > 256, NULL pointers, a negative workspace size
BAD = [dict(m=-1), dict(kdim=-1), dict(ncols=-1), dict(k=0), dict(k=-3), dict(k=257), dict(k=1040), dict(group_rows=0), dict(group_rows=-32),
       dict(group_rows=16), dict(group_rows=48), dict(group_rows=(1 << 41)), dict(labels=None), dict(g=None), dict(ws_bytes=-1), dict(m=1 << 41)]


@pytest.mark.parametrize("kw", BAD + [dict(centers=None), dict(dx=None)])
def test_dx_bad_arguments_are_einval_without_a_device(lib, kw):
    assert dx_call(lib, **kw) == NNC_EINVAL
    assert lib.nnc_last_error()


@pytest.mark.parametrize("kw", BAD + [dict(x=None), dict(dc=None), dict(ws=None), dict(ws=P + 4)])
def test_dc_bad_arguments_are_einval_without_a_device(lib, kw):
    assert dc_call(lib, **kw) == NNC_EINVAL
    assert lib.nnc_last_error()


def test_workspaces(lib):
    need = lib.nnc_cbmm_grouped_dx_workspace_bytes(1, 5000, 5000)
    assert need == lib.nnc_cbmm_dx_workspace_bytes(1, 5000, 5000, 1) > 0
    assert dx_call(lib, m=1, kdim=5000, ncols=5000, ws=P, ws_bytes=need - 1) == NNC_ENOSPACE
    assert dx_call(lib, m=1, kdim=5000, ncols=5000, ws=None, ws_bytes=need) == NNC_EINVAL
    for m, kdim, ncols, k, gr in [(1, 5000, 5000, 256, 32), (16, 112, 70, 16, 32), (300, 4096, 4096, 16, 128), (17, 20, 50, 3, 32)]:
        G = -(-kdim // gr)
        assert lib.nnc_cbmm_grouped_dc_workspace_bytes(m, kdim, ncols, k, gr) == 64 + 8 * G * k
    need = lib.nnc_cbmm_grouped_dc_workspace_bytes(1, 5000, 5000, 256, 32)
    assert dc_call(lib, m=1, kdim=5000, ncols=5000, k=256, ws_bytes=need - 1) == NNC_ENOSPACE
    for m, kdim, ncols in [(0, 5, 5), (3, 0, 5), (3, 5, 0), (30, 5, 0)]:
        assert lib.nnc_cbmm_grouped_dx_workspace_bytes(m, kdim, ncols) == 0 and lib.nnc_cbmm_grouped_dc_workspace_bytes(m, kdim, ncols, 4, 32) == 0


def test_huge_products_and_bin_counts_are_einval(lib):
    assert dc_call(lib, m=4, kdim=1 << 30, ncols=1 << 30, ws_bytes=1 << 20) == NNC_EINVAL
    out = (ctypes.c_int64 * nat.CBGRAD_GROUPED_PLAN_LEN)()
    assert lib.nnc_cbmm_grouped_dc_plan(4, 1 << 30, 1 << 30, 16, 32, 256, 0, out) == NNC_EINVAL
    assert lib.nnc_cbmm_grouped_dc_plan(4, 1 << 40, 4, 256, 32, 256, 0, out) == NNC_EINVAL      # 2^35 groups of 256 bins


@pytest.mark.parametrize("plan", [ops.cbmm_grouped_dx_plan, ops.cbmm_grouped_dc_plan])
def test_plan_argument_errors(lib, plan):
    for bad in [(4, 64, 16, 16, 32, 0), (4, 64, 16, 300, 32, 64), (4, 64, 16, 16, 48, 64), (4, 64, 16, 0, 32, 64), (-1, 64, 16, 16, 32, 64)]:
        with pytest.raises(nat.NncError):
            plan(*bad)
    assert lib.nnc_cbmm_grouped_dx_plan(4, 64, 16, 16, 32, 64, 0, None) == NNC_EINVAL
    assert lib.nnc_cbmm_grouped_dc_plan(4, 64, 16, 16, 32, 64, 0, None) == NNC_EINVAL


@pytest.mark.parametrize("case", ref.ALL_CASES, ids=[ref.case_id(c) for c in ref.ALL_CASES])
def test_the_plans_are_the_ungrouped_plans(lib, case):
    m, kdim, ncols, k, gr, off = (case[n] for n in ("m", "kdim", "ncols", "k", "group_rows", "off"))
    for cus in ref.CU_COUNTS:
        addr = 256 + off
        dx, dc = ops.cbmm_grouped_dx_plan(m, kdim, ncols, k, gr, cus, addr), ops.cbmm_grouped_dc_plan(m, kdim, ncols, k, gr, cus, addr)
        udx, udc = ops.cbmm_dx_plan(m, kdim, ncols, 1, k, cus, addr), ops.cbmm_dc_plan(m, kdim, ncols, 1, k, cus, addr)
        assert {f: dx[f] for f in ref.DX_SHARED} == {f: udx[f] for f in ref.DX_SHARED}
        assert {f: dc[f] for f in ref.DC_SHARED} == {f: udc[f] for f in ref.DC_SHARED}
        assert dx["workspace"] == lib.nnc_cbmm_grouped_dx_workspace_bytes(m, kdim, ncols)
        assert dc["workspace"] == lib.nnc_cbmm_grouped_dc_workspace_bytes(m, kdim, ncols, k, gr)
        if m * kdim * ncols:
            assert dc["terms_log2"] == math.ceil(math.log2(kdim * ncols * dc["splits"]))     # the whole layer's
            assert dc["workspace"] == 64 + 8 * ref.groups_of(case) * k
        for p in (dx, dc):
            assert p["group_rows"] == gr and p["groups"] == -(-kdim // gr)
            if p["path"] == ref.PATH_STREAM:
                rpg = p["rows_per_group"]
                assert rpg >= 1 and -(-kdim // rpg) == p["row_tiles"]
                assert p["max_groups_per_workgroup"] == ref.max_groups(kdim, rpg, kdim, gr)
            elif p["path"] == ref.PATH_TILED:
                assert p["rows_per_group"] == 0 and p["max_groups_per_workgroup"] == ref.max_groups(kdim, 128, kdim, gr)
                assert p["lds"] <= 64 * 1024
            else:
                assert p["rows_per_group"] == 0 and p["max_groups_per_workgroup"] == 0
        if dx["path"] == ref.PATH_TILED:
            tables = dx["copies"]
            assert tables in (1, 2, 4) and dx["lds"] == udx["lds"] + (tables - 1) * (k + 1) * 4
            assert dc["lds"] == udc["lds"] and udc["copies"] % dc["copies"] == 0 and udc["copies"] // dc["copies"] == tables
        elif dx["path"] == ref.PATH_STREAM:
            assert (dx["copies"], dx["entries"], dx["lds"]) == (udx["copies"], udx["entries"], udx["lds"])
            assert (dc["copies"], dc["lds"]) == (udc["copies"], udc["lds"])


def test_the_case_list_covers_the_regimes_it_claims(lib):
    """At 256 CUs: every fact the comments of the case list state, and between them every path, split and alignment."""
    seen = set()
    for case in ref.ALL_CASES:
        m, kdim, ncols, k, gr, off = (case[n] for n in ("m", "kdim", "ncols", "k", "group_rows", "off"))
        plans = {"dx": ops.cbmm_grouped_dx_plan(m, kdim, ncols, k, gr, 256, 256 + off), "dc": ops.cbmm_grouped_dc_plan(m, kdim, ncols, k, gr, 256, 256 + off)}
        for key, want in ref.EXPECT.get(ref.case_id(case), {}).items():
            which, field = key.split(":")
            assert plans[which][field] == want, (ref.case_id(case), key, plans[which][field], want)
        for which, p in plans.items():
            seen.add((which, p["path"], p["splits"] > 1, p["aligned"], min(p["max_groups_per_workgroup"], 3)))
    assert set(ref.EXPECT) == {ref.case_id(c) for c in ref.CASES}
    paths = {(w, p) for w, p, *_ in seen}
    assert paths == {("dx", ref.PATH_STREAM), ("dx", ref.PATH_TILED), ("dx", ref.PATH_NONE), ("dx", ref.PATH_ZERO),
                     ("dc", ref.PATH_STREAM), ("dc", ref.PATH_TILED), ("dc", ref.PATH_ZERO)}
    for which in ("dx", "dc"):
        for path in (ref.PATH_STREAM, ref.PATH_TILED):
            mg = {g for w, p, _, _, g in seen if (w, p) == (which, path)}
            assert {1, 2, 3} <= mg, (which, path, mg)                  # one group, one boundary, several in a workgroup
        assert {a for w, p, _, a, _ in seen if (w, p) == (which, ref.PATH_STREAM)} == {0, 1}
    assert {s for w, p, s, _, _ in seen if w == "dx" and p == ref.PATH_STREAM} == {False, True}
    assert {s for w, p, s, _, _ in seen if w == "dx" and p == ref.PATH_TILED} == {False, True}
    assert {s for w, p, s, _, _ in seen if w == "dc" and p == ref.PATH_TILED} == {False, True}


@pytest.mark.parametrize("m,kdim,ncols", [(1, 32, 1), (16, 5000, 5000), (1 << 40, 32, 1), (4096, 1 << 27, 1 << 28), (1 << 20, 1 << 20, 1 << 20 >> 6),
                                          (300, 8192, 8192)])
@pytest.mark.parametrize("ax,ag", [(1.0, 1.0), (3.4e38, 1e-30), (1e-30, 1e-30), (2.0 ** 60, 2.0 ** -3), (65504.0, 65504.0)])
def test_the_bound_keeps_the_integer_sums_in_int64(m, kdim, ncols, ax, ag):
    """A group's bins take at most the layer's 2^T images of at most 2^(P + S) each: |sum| <= 2^62, as for the ungrouped call."""
    try:
        plan = ops.cbmm_grouped_dc_plan(m, kdim, ncols, 256, 32, 256)
    except nat.NncError:
        assert kdim * ncols > (1 << 55) or max(m, kdim, ncols) > (1 << 40) or -(-kdim // 32) * 256 > (1 << 30)
        return
    t = plan["terms_log2"]
    assert t == ops.cbmm_dc_plan(m, kdim, ncols, 1, 256, 256)["terms_log2"]
    assert (1 << t) >= kdim * ncols * plan["splits"]
    S, flag = ops.cbgrad_shift(m, ax, ag, t)
    if flag != ops.CBGRAD_OK:
        return
    bound = Fraction(float(m) * float(np.float32(ax)) * float(np.float32(ag)))
    Pw = 62 - t - S
    assert Fraction(2) ** Pw > bound
    assert (kdim * ncols * plan["splits"]) * Fraction(2) ** (Pw + S) <= Fraction(2) ** 62
