"""CPU checks of the C ABI of the group-wise layer's backward pass from the bitmap-sparse form (include/nnc_cbspgrad_grouped.h,
nnc_cbsp_grouped_dx_* / nnc_cbsp_grouped_dc_*): the symbols, both plans against nnc_cbsp_dx_plan /
nnc_cbsp_dc_plan over CU counts with their added fields against NumPy counts, the workspace queries, every argument error with its
message (returned before any HIP call, so none of this needs a device), the Python doors that need no device, and the regimes and
group walks the shared case list claims at 256 CUs."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from neural_network_compression_amd import ops
from tests.helpers import grouped_sparse_grad_ref as ref

NNC_EINVAL, NNC_ENOSPACE = -1, -2
SYMBOLS = ("nnc_cbsp_grouped_dx_workspace_bytes", "nnc_cbsp_grouped_dx_plan", "nnc_cbsp_grouped_dx_f32",
           "nnc_cbsp_grouped_dc_workspace_bytes", "nnc_cbsp_grouped_dc_plan", "nnc_cbsp_grouped_dc_f32")
P = 0x1000   # a fake, never dereferenced, 256-byte aligned address


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_symbols_are_declared_exported_and_bound(lib):
    raw = ctypes.CDLL(nat.lib_path())
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(inc, "nnc_cbspgrad_grouped.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(nnc_[a-z0-9_]+)\s*\(", text)) == set(SYMBOLS) == set(nat.GROUPED_SPARSE_GRAD_SIGNATURES)
    assert '#include "nnc_cbspgrad_grouped.h"' in open(os.path.join(inc, "nnc.h")).read()
    protos = re.findall(r"^(int64_t|int)\s+(nnc_\w+)\s*\(([^;]*)\);", text, flags=re.M)
    assert {p[1] for p in protos} == set(SYMBOLS)
    ctype_of = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "int": ctypes.c_int}
    for res, name, args in protos:   # the declarations, argument by argument, against the bound signatures
        want = []
        for a in args.split(","):
            a = " ".join(a.split())
            if a == "int64_t *out":
                want.append(ctypes.POINTER(ctypes.c_int64))
            elif "*" in a:
                want.append(ctypes.c_void_p)
            else:
                want.append(ctype_of[a.rsplit(" ", 1)[0]])
        bound_res, bound_args = nat.GROUPED_SPARSE_GRAD_SIGNATURES[name]
        assert bound_res is ctype_of[res] and bound_args == want, name
        assert hasattr(raw, name) and getattr(lib, name).argtypes == bound_args and getattr(lib, name).restype is bound_res
    defs = {k: int(v) for k, v in re.findall(r"#define (NNC_\w+) (\d+)", text)}
    assert defs["NNC_CBSPDX_GROUPED_PLAN_LEN"] == nat.CBSPDX_GROUPED_PLAN_LEN == len(nat.CBSPDX_GROUPED_PLAN_FIELDS)
    assert defs["NNC_CBSPDC_GROUPED_PLAN_LEN"] == nat.CBSPDC_GROUPED_PLAN_LEN == len(nat.CBSPDC_GROUPED_PLAN_FIELDS)
    for name in ("group_rows", "groups", "rows_per_group", "max_groups_per_workgroup"):
        assert defs["NNC_CBSPDX_GROUPED_P_" + name.upper()] == nat.CBSPDX_GROUPED_PLAN_FIELDS.index(name)
        assert defs["NNC_CBSPDC_GROUPED_P_" + name.upper()] == nat.CBSPDC_GROUPED_PLAN_FIELDS.index(name)
    assert defs["NNC_CBSPDX_GROUPED_P_TABLES"] == nat.CBSPDX_GROUPED_PLAN_FIELDS.index("tables")
    assert nat.CBSPDX_GROUPED_PLAN_FIELDS[: nat.CBSPDX_PLAN_LEN] == nat.CBSPDX_PLAN_FIELDS
    assert nat.CBSPDC_GROUPED_PLAN_FIELDS[: nat.CBSPDC_PLAN_LEN] == nat.CBSPDC_PLAN_FIELDS
    assert not set(SYMBOLS) & (set(nat.SIGNATURES) | set(nat.GROUPED_SPARSE_SIGNATURES) | set(nat.GROUPED_GRAD_SIGNATURES))


# ------------------------------------------------------------------ the plans
def _tables(gr):
    return 1 if gr % 128 == 0 else (4 if gr == 32 else 2)


def _max_groups(spans, gr):
    return max((hi - 1) // gr - lo // gr + 1 for lo, hi in spans)


@pytest.mark.parametrize("case", ref.CASES, ids=ref.IDS)
def test_the_plans_are_the_ungrouped_sparse_plans(lib, case):
    m, kdim, ncols, k, gr = (case[n] for n in ("m", "kdim", "ncols", "k", "group_rows"))
    for cus in ref.CU_COUNTS:
        dx, dc = ops.cbsp_grouped_dx_plan(m, kdim, ncols, k, gr, cus), ops.cbsp_grouped_dc_plan(m, kdim, ncols, k, gr, cus)
        udx, udc = ops.cbsp_dx_plan(m, kdim, ncols, 1, k, cus), ops.cbsp_dc_plan(m, kdim, ncols, 1, k, cus)
        tiled = dx["path"] == ref.PATH_TILED
        for f in nat.CBSPDX_PLAN_FIELDS:
            if f != "lds":
                assert dx[f] == udx[f], (f, cus)
        for f in nat.CBSPDC_PLAN_FIELDS:
            if f != "workspace":
                assert dc[f] == udc[f], (f, cus)
        # LDS: the ungrouped figure, plus (TABLES - 1)(K + 1) words for tiled dx only
        assert dx["tables"] == (_tables(gr) if tiled else 0)
        assert dx["lds"] == udx["lds"] + ((dx["tables"] - 1) * (k + 1) * 4 if tiled else 0) <= 64 * 1024
        # the workspaces: section 13's for dx (partials 256-byte aligned, then m floats of row sums), section 19's for dc
        part = -(-dx["splits"] * m * kdim * 4 // 256) * 256 if dx["splits"] > 1 else 0
        assert dx["workspace"] == part + 4 * m
        assert dc["workspace"] == 64 + 8 * ref.groups_of(case) * k
        assert dc["terms_log2"] == math.ceil(math.log2(kdim * ncols * dc["splits"])) == ops.cbmm_dc_plan(m, kdim, ncols, 1, k, cus)["terms_log2"]
        for which, p in (("dx", dx), ("dc", dc)):
            assert p["group_rows"] == gr and p["groups"] == -(-kdim // gr)
            if p["path"] == ref.PATH_STREAM:
                rpg = p["rows_per_group"]
                assert rpg >= 1 and -(-kdim // rpg) == p["row_tiles"]
                spans = [(w * rpg, min(kdim, (w + 1) * rpg)) for w in range(p["row_tiles"])]
            else:
                assert p["path"] == ref.PATH_TILED and p["rows_per_group"] == 0
                spans = [(t, min(kdim, t + 128)) for t in range(0, kdim, 128)]
            assert p["max_groups_per_workgroup"] == _max_groups(spans, gr) <= (4 if p["path"] == ref.PATH_TILED else kdim)
            ref.features_of(case, which, p)   # (asserts that the walk it derives fits the plan)
    assert lib.nnc_cbsp_grouped_dx_workspace_bytes(m, kdim, ncols) == ops.cbsp_grouped_dx_plan(m, kdim, ncols, k, gr, 256)["workspace"]
    assert lib.nnc_cbsp_grouped_dx_workspace_bytes(m, kdim, ncols) == lib.nnc_cbsp_dx_workspace_bytes(m, kdim, ncols, 1)
    assert lib.nnc_cbsp_grouped_dc_workspace_bytes(m, kdim, ncols, k, gr) == 64 + 8 * ref.groups_of(case) * k


@pytest.mark.parametrize("m,kdim,ncols", ref.EMPTY)
def test_empty_shapes_plan_as_the_ungrouped_calls(lib, m, kdim, ncols):
    dx, dc = ops.cbsp_grouped_dx_plan(m, kdim, ncols, 16, 32, 256), ops.cbsp_grouped_dc_plan(m, kdim, ncols, 16, 32, 256)
    assert dx["path"] == (ref.PATH_NONE if m == 0 or kdim == 0 else ref.PATH_ZERO) == ops.cbsp_dx_plan(m, kdim, ncols, 1, 16, 256)["path"]
    assert dc["path"] == ref.PATH_ZERO and dx["workspace"] == dc["workspace"] == 0 and dx["tables"] == 0
    assert lib.nnc_cbsp_grouped_dx_workspace_bytes(m, kdim, ncols) == lib.nnc_cbsp_grouped_dc_workspace_bytes(m, kdim, ncols, 16, 32) == 0
    assert dx["groups"] == dc["groups"] == -(-kdim // 32) and dx["max_groups_per_workgroup"] == dc["max_groups_per_workgroup"] == 0


def test_the_case_list_hits_every_regime_and_group_walk_at_256_cus(lib):
    seen, feats = set(), set()
    for c in ref.CASES:
        dx = ops.cbsp_grouped_dx_plan(c["m"], c["kdim"], c["ncols"], c["k"], c["group_rows"], 256)
        dc = ops.cbsp_grouped_dc_plan(c["m"], c["kdim"], c["ncols"], c["k"], c["group_rows"], 256)
        seen |= ref.regimes_of(dx, dc)
        feats |= ref.features_of(c, "dx", dx) | ref.features_of(c, "dc", dc)
    for m, kdim, ncols in ref.EMPTY:
        seen |= ref.regimes_of(ops.cbsp_grouped_dx_plan(m, kdim, ncols, 16, 32, 256), ops.cbsp_grouped_dc_plan(m, kdim, ncols, 16, 32, 256))
    assert ref.required_regimes() <= seen, ref.required_regimes() - seen
    assert ref.required_features() <= feats, ref.required_features() - feats
    assert {c["ncols"] for c in ref.CASES} >= {1, 50, 64, 65, 130} and {c["k"] for c in ref.CASES} == {3, 16, 256}
    assert any(c["off"] % 2 for c in ref.CASES) and any(c["pruned"] for c in ref.CASES)
    assert max(c["kdim"] for c in ref.CASES) <= 2100 and max(c["ncols"] for c in ref.CASES) <= 1100 and max(c["m"] for c in ref.CASES) <= 260


def test_the_case_data_covers_the_group_kinds_and_is_exact():
    """Entirely pruned groups, groups at density 1.0, z_q >= K, stored labels >= K, c_{z_q} == 0 and != 0, a different z per group,
    nnz = 0; exact_data asserts the 2^24 quarter-unit bound itself, and on exact data the formula is g @ W^T."""
    kinds = set()
    for ci, c in enumerate(ref.CASES):
        lab, zs, x, g, cen = ref.exact_data(c, 300 + ci, ci)
        kept = ref.fwd.keep_mask(lab, zs, c["group_rows"])
        cz = ref.fwd.cz_of(cen, zs)
        kinds |= {"nnz 0"} if not kept.any() else set()
        for q, z in enumerate(zs):
            rows = slice(q * c["group_rows"], (q + 1) * c["group_rows"])
            share = kept[rows].mean()
            kinds |= {"pruned"} if share == 0 else ({"full"} if share == 1 else set())
            kinds |= {"z past K"} if z >= c["k"] else set()
            kinds |= {"stored label past K"} if (lab[rows][kept[rows]] >= c["k"]).any() else set()
            kinds |= {"cz zero"} if cz[q] == 0 else {"cz non-zero"}
        if len(zs) > 1:
            assert len(set(zs.tolist())) > 1
        want = ref.dx64(g, lab, cen, zs, c["group_rows"])
        w = ref.grouped_ref.weights(cen, lab, c["kdim"], c["ncols"], c["group_rows"]).astype(np.float64)
        assert np.array_equal(want, g.astype(np.float64) @ w.T)
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
        r64, bound = ref.dx_bound(g, lab, cen, zs, c["group_rows"])
        assert np.array_equal(r64, want) and np.all(bound > 0)
    assert kinds == {"pruned", "full", "z past K", "stored label past K", "cz zero", "cz non-zero", "nnz 0"}


# ------------------------------------------------------------------ argument errors, all before any HIP call
def dx_call(lib, g=P, m=4, kdim=64, packed=P, packed_bytes=None, ncols=16, zs=P, nnz=10, centers=P, k=16, group_rows=32, dx=P, ws=P, ws_bytes=None):
    ok = min(m, kdim, ncols) >= 0
    if packed_bytes is None:
        packed_bytes = lib.nnc_cbsp_pack_bytes(kdim, ncols, 1, max(nnz, 0)) if ok else 0
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbsp_grouped_dx_workspace_bytes(m, kdim, ncols) if ok else 0
    return lib.nnc_cbsp_grouped_dx_f32(g, m, kdim, packed, packed_bytes, ncols, zs, nnz, centers, k, group_rows, dx, ws, ws_bytes, None)


def dc_call(lib, x=P, g=P, m=4, kdim=64, packed=P, packed_bytes=None, ncols=16, zs=P, nnz=10, k=16, group_rows=32, dc=P, f64=1, ws=P, ws_bytes=None):
    ok = min(m, kdim, ncols) >= 0
    if packed_bytes is None:
        packed_bytes = lib.nnc_cbsp_pack_bytes(kdim, ncols, 1, max(nnz, 0)) if ok else 0
    if ws_bytes is None:
        good = ok and 1 <= k <= 256 and group_rows >= 32 and group_rows % 32 == 0
        ws_bytes = lib.nnc_cbsp_grouped_dc_workspace_bytes(m, kdim, ncols, k, group_rows) if good else 0
    return lib.nnc_cbsp_grouped_dc_f32(x, g, m, kdim, packed, packed_bytes, ncols, zs, nnz, k, group_rows, dc, f64, ws, ws_bytes, None)


# (arguments, what the message says)
BAD = [(dict(m=-1), "negative size"), (dict(kdim=-1), "negative size"), (dict(ncols=-1), "negative size"), (dict(m=1 << 41), "size too large"),
       (dict(ncols=1 << 32), "size too large"), (dict(k=0), "k outside 1..NNC_KMAX"), (dict(k=-3), "k outside 1..NNC_KMAX"),
       (dict(k=257), "k outside 1..256"), (dict(k=1040), "k outside 1..256"),
       (dict(group_rows=0), "group_rows must be a positive multiple of 32"), (dict(group_rows=-32), "group_rows must be a positive multiple of 32"),
       (dict(group_rows=16), "group_rows must be a positive multiple of 32"), (dict(group_rows=48), "group_rows must be a positive multiple of 32"),
       (dict(group_rows=1 << 41), "size too large"), (dict(nnz=-1), "nnz outside 0..kdim * ncols"), (dict(nnz=64 * 16 + 1), "nnz outside 0..kdim * ncols"),
       (dict(packed_bytes=100), "packed buffer smaller than nnc_cbsp_pack_bytes(kdim, ncols, 1, nnz)"), (dict(packed=None), "packed or zero_symbols is NULL"),
       (dict(zs=None), "packed or zero_symbols is NULL"), (dict(packed=P + 8), "packed must be 256-byte aligned"),
       (dict(ws_bytes=-1), "negative workspace size"), (dict(ws=None), "workspace is NULL")]


def _message(lib):
    return lib.nnc_last_error().decode()


@pytest.mark.parametrize("kw,msg", BAD + [(dict(g=None), "g is NULL"), (dict(centers=None), "centers is NULL"), (dict(dx=None), "dx is NULL"),
                                          (dict(ws=P + 2), "workspace must be 4-byte aligned")], ids=lambda v: str(v) if isinstance(v, dict) else "")
def test_dx_bad_arguments_are_einval_without_a_device(lib, kw, msg):
    assert dx_call(lib, **kw) == NNC_EINVAL
    assert _message(lib).startswith("nnc_cbsp_grouped_dx_f32: ") and msg in _message(lib)


@pytest.mark.parametrize("kw,msg", BAD + [(dict(x=None), "x or g is NULL"), (dict(g=None), "x or g is NULL"), (dict(dc=None), "dc is NULL"),
                                          (dict(ws=P + 4), "workspace not 8-byte aligned")], ids=lambda v: str(v) if isinstance(v, dict) else "")
def test_dc_bad_arguments_are_einval_without_a_device(lib, kw, msg):
    assert dc_call(lib, **kw) == NNC_EINVAL
    assert _message(lib).startswith("nnc_cbsp_grouped_dc_f32: ") and msg in _message(lib)


def test_short_workspaces_are_enospace_and_bin_counts_are_bounded(lib):
    need = lib.nnc_cbsp_grouped_dx_workspace_bytes(4, 64, 16)
    assert need == 4 * 4                                               # a direct call still needs the row sums
    assert dx_call(lib, ws_bytes=need - 1) == NNC_ENOSPACE and "workspace smaller than nnc_cbsp_grouped_dx_workspace_bytes()" in _message(lib)
    need = lib.nnc_cbsp_grouped_dx_workspace_bytes(1, 600, 1030)
    assert need > 256 and dx_call(lib, m=1, kdim=600, ncols=1030, ws_bytes=need - 1) == NNC_ENOSPACE   # partials in front of the row sums
    need = lib.nnc_cbsp_grouped_dc_workspace_bytes(4, 64, 16, 16, 32)
    assert need == 64 + 8 * 2 * 16
    assert dc_call(lib, ws_bytes=need - 1) == NNC_ENOSPACE and "workspace smaller than nnc_cbsp_grouped_dc_workspace_bytes()" in _message(lib)
    out = (ctypes.c_int64 * nat.CBSPDC_GROUPED_PLAN_LEN)()
    assert lib.nnc_cbsp_grouped_dc_plan(4, 1 << 32, 4, 256, 32, 256, out) == NNC_EINVAL and "more than 2^30 bins" in _message(lib)   # 2^27 groups of 256 bins
    assert lib.nnc_cbsp_grouped_dc_workspace_bytes(4, 1 << 32, 4, 256, 32) == 0
    for m, kdim, ncols in ref.EMPTY + [(-1, 5, 5)]:
        assert lib.nnc_cbsp_grouped_dx_workspace_bytes(m, kdim, ncols) == 0 and lib.nnc_cbsp_grouped_dc_workspace_bytes(m, kdim, ncols, 4, 32) == 0


def test_empty_dx_calls_need_no_device(lib):
    """m = 0 or kdim = 0: dx is empty, NNC_OK with no pointer touched and no launch."""
    assert dx_call(lib, m=0, g=None, dx=None, ws=None, packed=None, zs=None, ws_bytes=0) == 0
    assert dx_call(lib, kdim=0, nnz=0, g=None, dx=None, ws=None, packed=None, zs=None, ws_bytes=0) == 0


@pytest.mark.parametrize("plan,length", [(ops.cbsp_grouped_dx_plan, nat.CBSPDX_GROUPED_PLAN_LEN), (ops.cbsp_grouped_dc_plan, nat.CBSPDC_GROUPED_PLAN_LEN)])
def test_plan_argument_errors(lib, plan, length):
    for bad in [(4, 64, 16, 16, 32, 0), (4, 64, 16, 300, 32, 64), (4, 64, 16, 16, 48, 64), (4, 64, 16, 0, 32, 64), (-1, 64, 16, 16, 32, 64),
                (4, -1, 16, 16, 32, 64), (4, 64, -1, 16, 32, 64)]:
        with pytest.raises(nat.NncError):
            plan(*bad)
    assert lib.nnc_cbsp_grouped_dx_plan(4, 64, 16, 16, 32, 64, None) == NNC_EINVAL and "out is NULL" in _message(lib)
    assert lib.nnc_cbsp_grouped_dc_plan(4, 64, 16, 16, 32, 64, None) == NNC_EINVAL and "out is NULL" in _message(lib)
    assert len(plan(4, 64, 16, 16, 32, 64)) == length


# ------------------------------------------------------------------ the Python doors that need no device
class _Net:
    def get_config(self):
        return {}


def test_the_python_doors_refuse_before_any_device_work():
    from neural_network_compression_amd import compressed
    from neural_network_compression_amd.common import trainer as tr

    for bad in (None, "yes", 2, 0.5):
        with pytest.raises(ValueError, match="sparse must be False, True or 'auto'"):
            compressed.compress_network_trainable_grouped(_Net(), {}, sparse=bad)
    for option in (True, "auto"):
        with pytest.raises(ValueError, match="sparse needs half_inputs=False"):
            compressed.compress_network_trainable_grouped(_Net(), {}, sparse=option, half_inputs=True)
    with pytest.raises(ValueError, match="sparse=True and packed=True both ask for every layer"):
        compressed.compress_network_trainable_grouped(_Net(), {}, sparse=True, packed=True)
    with pytest.raises(ValueError, match="packed must be False, True or 'auto'"):
        compressed.compress_network_trainable_grouped(_Net(), {}, sparse=True, packed="yes")
    import torch

    t = types.SimpleNamespace(quantized_models_by_layer={"a": 1})
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(ValueError, match="sparse needs activation_dtype=None"):
            tr.Trainer.fine_tune_grouped(t, None, None, 1, sparse=True, activation_dtype=dt)
    # the ops: a codes object of the wrong kind, and half activations, before any tensor is looked at
    with pytest.raises(TypeError, match="GroupedSparseCodes"):
        ops.grouped_sparse_codebook_linear(None, object(), None)
    assert hasattr(compressed, "TrainableGroupedSparseCompressedDense")
    for name in ("from_dense", "from_codes", "from_grouped", "from_grouped_sparse"):
        assert callable(getattr(compressed.TrainableGroupedSparseCompressedDense, name))
