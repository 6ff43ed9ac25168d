"""CPU checks of the C ABI of the group-wise layer's bitmap-sparse form (include/nnc_cbsp_grouped.h, nnc_cbsp_grouped_*; DESIGN.md
section 28): the symbols, the plan against nnc_cbsp_plan over CU counts with its three added fields, the workspace, the argument
errors (returned before any HIP call, so none of this needs a device), the regimes and boundary walks the shared case list claims,
and the exactness bound of its exact data."""
import ctypes
import os
import re

import numpy as np
import pytest

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from neural_network_compression_amd import ops
from tests.helpers import grouped_sparse_ref as ref
from tests.helpers import sparse_ref

NNC_EINVAL, NNC_ENOSPACE = -1, -2
SYMBOLS = ("nnc_cbsp_grouped_pack", "nnc_cbsp_grouped_unpack", "nnc_cbsp_grouped_workspace_bytes", "nnc_cbsp_grouped_plan", "nnc_cbsp_grouped_f32")
P = 0x1000   # a fake, never dereferenced, 256-byte aligned address
CBSP_ROWSUM_PASS = 2


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_symbols_are_declared_exported_and_bound(lib):
    raw = ctypes.CDLL(nat.lib_path())
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "nnc_cbsp_grouped.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(nnc_[a-z0-9_]+)\s*\(", text)) == set(SYMBOLS) == set(nat.GROUPED_SPARSE_SIGNATURES)
    assert '#include "nnc_cbsp_grouped.h"' in open(os.path.join(inc, "nnc.h")).read()
    for s in SYMBOLS:
        assert hasattr(raw, s) and getattr(lib, s).argtypes == nat.GROUPED_SPARSE_SIGNATURES[s][1]
    defs = {k: int(v) for k, v in re.findall(r"#define (NNC_\w+) (\d+)", text)}
    assert defs["NNC_CBSP_GROUPED_PLAN_LEN"] == nat.CBSP_GROUPED_PLAN_LEN == len(nat.CBSP_GROUPED_PLAN_FIELDS)
    for name in ("group_rows", "groups", "max_groups_per_split"):
        assert defs["NNC_CBSP_GROUPED_P_" + name.upper()] == nat.CBSP_GROUPED_PLAN_FIELDS.index(name)
    assert nat.CBSP_GROUPED_PLAN_FIELDS[: nat.CBSP_PLAN_LEN] == nat.CBSP_PLAN_FIELDS


@pytest.mark.parametrize("case", ref.CASES, ids=[ref.case_id(c) for c in ref.CASES])
def test_the_plan_is_the_ungrouped_sparse_plan(lib, case):
    m, kdim, ncols, k, gr = (case[n] for n in ("m", "kdim", "ncols", "k", "group_rows"))
    for cus in ref.CU_COUNTS:
        got = ops.cbsp_grouped_plan(m, kdim, ncols, k, gr, cus)
        want = ops.cbsp_plan(m, kdim, ncols, 1, k, cus)
        for f in nat.CBSP_PLAN_FIELDS:
            if f not in ("rowsum", "workspace"):
                assert got[f] == want[f], (f, cus)
        assert got["rowsum"] == CBSP_ROWSUM_PASS
        assert got["group_rows"] == gr and got["groups"] == -(-kdim // gr)
        ranges = ref.split_ranges(got, kdim)
        assert ranges[0][0] == 0 and ranges[-1][1] == kdim and all(hi > lo for lo, hi in ranges)
        assert got["max_groups_per_split"] == max((hi - 1) // gr - lo // gr + 1 for lo, hi in ranges)
        # the workspace: the partials (256-byte aligned), then t (m floats), then the word that says whether t applies
        part = -(-got["splits"] * m * ncols * 4 // 256) * 256 if got["splits"] > 1 else 0
        assert got["workspace"] == part + 4 * m + 4
        assert lib.nnc_cbsp_grouped_workspace_bytes(m, kdim, ncols) >= got["workspace"]
    assert lib.nnc_cbsp_grouped_workspace_bytes(m, kdim, ncols) == ops.cbsp_grouped_plan(m, kdim, ncols, k, gr, 256)["workspace"]


def test_the_case_list_hits_every_regime_and_boundary_walk_at_256_cus(lib):
    seen, feats = set(), set()
    for c in ref.CASES:
        plan = ops.cbsp_grouped_plan(c["m"], c["kdim"], c["ncols"], c["k"], c["group_rows"], 256)
        seen.add(ref.regime_of(plan))
        feats |= ref.features_of(c, plan)
    assert ref.required_regimes() <= seen, ref.required_regimes() - seen
    assert ref.required_features() <= feats, ref.required_features() - feats
    assert {c["ncols"] for c in ref.CASES} >= {1, 50, 64, 130} and {c["k"] for c in ref.CASES} == {3, 16, 256}
    assert any(c["off"] % 2 for c in ref.CASES) and any(c["x_view"] for c in ref.CASES) and {c["bias"] for c in ref.CASES} == {True, False}


def test_the_case_data_covers_the_group_kinds_and_is_exact():
    """Entirely pruned groups, groups at density 1.0, z_g >= K, stored labels >= K, c_{z_g} == 0 and != 0, different z per group;
    exact_data asserts the 2^24 quarter-unit bound itself."""
    kinds = set()
    for ci, c in enumerate(ref.CASES):
        lab, zs, x, cen, bias = ref.exact_data(c, 100 + ci, ci)
        kept = ref.keep_mask(lab, zs, c["group_rows"])
        cz = ref.cz_of(cen, zs)
        for g, z in enumerate(zs):
            rows = slice(g * c["group_rows"], (g + 1) * c["group_rows"])
            share = kept[rows].mean()
            kinds |= {"pruned"} if share == 0 else ({"full"} if share == 1 else set())
            kinds |= {"z past K"} if z >= c["k"] else set()
            kinds |= {"stored label past K"} if (lab[rows][kept[rows]] >= c["k"]).any() else set()
            kinds |= {"cz zero"} if cz[g] == 0 else {"cz non-zero"}
        if len(zs) > 1:
            assert len(set(zs.tolist())) > 1
        ref64 = ref.formula64(x, lab, cen, zs, c["group_rows"], bias)
        w = ref.grouped_ref.weights(cen, lab, c["kdim"], c["ncols"], c["group_rows"])
        assert np.array_equal(ref64, ref.grouped_ref.reference(x, w, bias))   # the formula is x @ W on exact data
        assert np.array_equal(ref64.astype(np.float32).astype(np.float64), ref64)
    assert kinds == {"pruned", "full", "z past K", "stored label past K", "cz zero", "cz non-zero"}


def test_pack_np_is_sparse_ref_pack_np_with_one_group():
    rng = np.random.RandomState(3)
    lab = sparse_ref.labels_at_density(rng, 40, 70, 16, 0.2, 5)
    a, b = ref.pack_np(lab, 40, 70, 64, np.array([5], dtype=np.uint8)), sparse_ref.pack_np(lab, 40, 70, 5)
    assert a["nnz"] == b["nnz"] and all(np.array_equal(a[f], b[f]) for f in ("bitmap", "counts", "symbols"))


# ------------------------------------------------------------------ argument errors, all before any HIP call
def f32_call(lib, x=P, m=4, kdim=64, packed=P, packed_bytes=None, ncols=16, zs=P, nnz=10, centers=P, k=16, group_rows=32, y=P, ws=P, ws_bytes=None):
    ok = min(m, kdim, ncols) >= 0
    if packed_bytes is None:
        packed_bytes = lib.nnc_cbsp_pack_bytes(kdim, ncols, 1, nnz) if ok else 0
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbsp_grouped_workspace_bytes(m, kdim, ncols) if ok else 0
    return lib.nnc_cbsp_grouped_f32(x, m, kdim, packed, packed_bytes, ncols, zs, nnz, centers, k, group_rows, None, 0, y, ws, ws_bytes, None)


def pack_call(lib, labels=P, kdim=64, ncols=16, group_rows=32, zs=P, packed=P, packed_bytes=None):
    if packed_bytes is None:
        packed_bytes = lib.nnc_cbsp_pack_bytes(kdim, ncols, 1, 0) if min(kdim, ncols) >= 0 else 0
    return lib.nnc_cbsp_grouped_pack(labels, kdim, ncols, group_rows, zs, packed, packed_bytes, None, None)


def unpack_call(lib, packed=P, packed_bytes=None, kdim=64, ncols=16, group_rows=32, zs=P, nnz=10, out=P):
    if packed_bytes is None:
        packed_bytes = lib.nnc_cbsp_pack_bytes(kdim, ncols, 1, max(nnz, 0)) if min(kdim, ncols) >= 0 else 0
    return lib.nnc_cbsp_grouped_unpack(packed, packed_bytes, kdim, ncols, group_rows, zs, nnz, out, None)


BAD_ROWS = [dict(group_rows=0), dict(group_rows=-32), dict(group_rows=16), dict(group_rows=48), dict(group_rows=(1 << 41))]


@pytest.mark.parametrize("kw", BAD_ROWS + [dict(m=-1), dict(kdim=-1), dict(ncols=-1), dict(m=1 << 41), dict(k=0), dict(k=-3), dict(k=257), dict(k=1040),
                                           dict(nnz=-1), dict(nnz=64 * 16 + 1), dict(packed_bytes=100), dict(packed=P + 8), dict(packed=None),
                                           dict(x=None), dict(zs=None), dict(centers=None), dict(y=None), dict(ws=None), dict(ws=P + 2),
                                           dict(ws_bytes=-1), dict(ncols=1 << 32)])
def test_f32_bad_arguments_are_einval_without_a_device(lib, kw):
    assert f32_call(lib, **kw) == NNC_EINVAL
    assert lib.nnc_last_error()


@pytest.mark.parametrize("kw", BAD_ROWS + [dict(kdim=-1), dict(ncols=-1), dict(packed=P + 8), dict(packed=None), dict(labels=None), dict(zs=None),
                                           dict(ncols=1 << 32)])
def test_pack_bad_arguments_are_einval_without_a_device(lib, kw):
    assert pack_call(lib, **kw) == NNC_EINVAL
    assert lib.nnc_last_error()


@pytest.mark.parametrize("kw", BAD_ROWS + [dict(kdim=-1), dict(ncols=-1), dict(nnz=-1), dict(nnz=64 * 16 + 1), dict(packed_bytes=100), dict(packed=P + 8),
                                           dict(packed=None), dict(out=None), dict(zs=None)])
def test_unpack_bad_arguments_are_einval_without_a_device(lib, kw):
    assert unpack_call(lib, **kw) == NNC_EINVAL
    assert lib.nnc_last_error()


def test_short_buffers_are_enospace(lib):
    assert pack_call(lib, packed_bytes=lib.nnc_cbsp_pack_bytes(64, 16, 1, 0) - 1) == NNC_ENOSPACE
    need = lib.nnc_cbsp_grouped_workspace_bytes(1, 5000, 300)
    assert need > 4 * 1 + 4                                           # a split call: partials in front of t
    assert f32_call(lib, m=1, kdim=5000, ncols=300, ws_bytes=need - 1) == NNC_ENOSPACE
    assert f32_call(lib, m=4, ws_bytes=4 * 4 + 3) == NNC_ENOSPACE     # a direct call still needs t and the word behind it
    for m, kdim, ncols in [(0, 5, 5), (3, 0, 5), (3, 5, 0), (-1, 5, 5)]:
        assert lib.nnc_cbsp_grouped_workspace_bytes(m, kdim, ncols) == 0


def test_empty_calls_need_no_device(lib):
    """m = 0 or ncols = 0 is a no-op: NNC_OK with no pointer touched and no launch."""
    assert f32_call(lib, m=0, x=None, y=None, ws=None, ws_bytes=0) == 0
    assert f32_call(lib, ncols=0, nnz=0, x=None, y=None, ws=None, ws_bytes=0) == 0
    assert unpack_call(lib, kdim=0, nnz=0, packed=None, out=None, zs=None) == 0


def test_plan_argument_errors(lib):
    for bad in [(4, 64, 16, 16, 32, 0), (4, 64, 16, 300, 32, 64), (4, 64, 16, 16, 48, 64), (4, 64, 16, 0, 32, 64), (-1, 64, 16, 16, 32, 64),
                (4, -1, 16, 16, 32, 64), (4, 64, -1, 16, 32, 64)]:
        with pytest.raises(nat.NncError):
            ops.cbsp_grouped_plan(*bad)
    assert lib.nnc_cbsp_grouped_plan(4, 64, 16, 16, 32, 64, None) == NNC_EINVAL
    empty = ops.cbsp_grouped_plan(0, 64, 16, 16, 32, 64)
    assert empty["path"] == 0 and empty["workspace"] == 0 and empty["rowsum"] == 0
    bias_only = ops.cbsp_grouped_plan(4, 0, 16, 16, 32, 64)
    assert bias_only["path"] == 3 and bias_only["groups"] == 0 and bias_only["workspace"] == 0
