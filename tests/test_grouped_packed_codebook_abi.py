"""CPU checks of the group-wise packed codebook matmul's C ABI (include/nnc.h, nnc_cbpk_grouped*): the plan
is the ungrouped packed one (nnc_cbpk_plan) for the stream and the tiled kernel and the MFMA grid of the byte-form grouped call for
half x at m > 16, plus the group fields; the case list of the GPU suite (tests/helpers/grouped_packed_ref.py) reaches every kernel
and every way of walking through groups at several CU counts; every argument error comes back before any HIP call, so none of this
needs a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from tests.helpers import cbmm_ref, grouped_packed_ref as gp, grouped_ref, packed_ref
from tests.helpers.grouped_packed_ref import CASES, CU_COUNTS, DTYPES

NNC_EINVAL, NNC_ENOSPACE = -1, -2
SHARED_WITH_PACKED = ("path", "vb", "mt", "cols", "xrows", "table", "copies", "entries", "splits", "rps", "col_tiles", "row_tiles", "workspace")
HALF = (nat.DT_BF16, nat.DT_F16)


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def gplan(lib, dt, m, kdim, ncols, bits, k, group_rows, cus):
    out = (ctypes.c_int64 * nat.CBPK_GROUPED_PLAN_LEN)()
    rc = lib.nnc_cbpk_grouped_plan(dt, m, kdim, ncols, bits, k, group_rows, cus, out)
    assert rc == 0, (dt, m, kdim, ncols, bits, k, group_rows, cus, lib.nnc_last_error())
    return dict(zip(nat.CBPK_GROUPED_PLAN_FIELDS, out))


def uplan(lib, m, kdim, ncols, bits, k, cus):
    out = (ctypes.c_int64 * nat.CBPK_PLAN_LEN)()
    assert lib.nnc_cbpk_plan(m, kdim, ncols, bits, k, cus, out) == 0
    return dict(zip(nat.CBPK_PLAN_FIELDS, out))


def byte_grouped_plan(lib, dt, m, kdim, ncols, k, group_rows, cus):
    out = (ctypes.c_int64 * nat.CBMM_GROUPED_PLAN_LEN)()
    assert lib.nnc_cbmm_grouped_plan(dt, m, kdim, ncols, k, group_rows, cus, 0, out) == 0
    return dict(zip(nat.CBMM_GROUPED_PLAN_FIELDS, out))


def test_symbols_header_and_signatures_agree(lib):
    raw = ctypes.CDLL(nat.lib_path())
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nnc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nnc_cbpk_grouped\w*)\s*\(", code))
    assert declared == {"nnc_cbpk_grouped", "nnc_cbpk_grouped_workspace_bytes", "nnc_cbpk_grouped_plan"}
    for s in declared:
        assert hasattr(raw, s) and s in nat.SIGNATURES, s
    defs = {k: int(v) for k, v in re.findall(r"#define (NNC_\w+) (\d+)", text)}
    assert defs["NNC_CBPK_GROUPED_PLAN_LEN"] == nat.CBPK_GROUPED_PLAN_LEN == len(nat.CBPK_GROUPED_PLAN_FIELDS)
    for name in ("dtype", "group_rows", "groups", "max_groups_per_split", "tables"):
        assert defs["NNC_CBPK_GROUPED_P_" + name.upper()] == nat.CBPK_GROUPED_PLAN_FIELDS.index(name)
    assert nat.CBPK_GROUPED_PLAN_FIELDS[: nat.CBPK_PLAN_LEN] == nat.CBPK_PLAN_FIELDS
    assert gp.DT_CODE == {"f32": nat.DT_F32, "bf16": nat.DT_BF16, "fp16": nat.DT_F16}
    assert (gp.PATH_STREAM, gp.PATH_TILED, gp.PATH_MFMA) == (nat.CBMM_STREAM, nat.CBMM_TILED, nat.CBMM_MFMA)


PLAN_MS = [0, 1, 3, 16, 17, 129, 4096]
PLAN_KDIMS = [0, 1, 33, 112, 300, 1001, 4096]
PLAN_NCOLS = [0, 1, 50, 130, 4096]
PLAN_ROWS = [32, 128, 1 << 20]


def test_plan_is_the_packed_plan_or_the_mfma_grid_plus_the_group_fields(lib):
    for dt in (nat.DT_F32,) + HALF:
        for bits, k in ((2, 3), (4, 16)):
            for m in PLAN_MS:
                for kdim in PLAN_KDIMS:
                    for ncols in PLAN_NCOLS:
                        ws = lib.nnc_cbpk_grouped_workspace_bytes(dt, m, kdim, ncols, bits)
                        query = gplan(lib, dt, m, kdim, ncols, bits, k, 32, 256)
                        assert ws == query["workspace"], (dt, bits, m, kdim, ncols)
                        last_splits = 0
                        for cus in CU_COUNTS:
                            u = uplan(lib, m, kdim, ncols, bits, k, cus)
                            for rows in PLAN_ROWS:
                                p = gplan(lib, dt, m, kdim, ncols, bits, k, rows, cus)
                                where = (dt, bits, m, kdim, ncols, k, rows, cus, p, u)
                                assert p["dtype"] == dt and p["group_rows"] == rows, where
                                assert p["groups"] == -(-kdim // rows), where
                                assert p["lds"] <= 64 * 1024, where
                                assert p["workspace"] == (p["splits"] * m * ncols * 4 if p["splits"] > 1 else 0) <= ws, where
                                if p["path"] in (nat.CBMM_NONE, nat.CBMM_BIAS):
                                    assert p["path"] == u["path"] and p["max_groups_per_split"] == 0 and p["tables"] == 0, where
                                    continue
                                spans = [(hi - 1) // rows - lo // rows + 1 for lo, hi in gp.split_ranges(p, kdim)]
                                assert p["max_groups_per_split"] == max(spans) >= 1, where
                                assert p["max_groups_per_split"] <= p["groups"], where
                                assert p["entries"] == 1 << bits, where
                                if dt in HALF and m > 16:
                                    b = byte_grouped_plan(lib, dt, m, kdim, ncols, k, rows, cus)
                                    assert p["path"] == b["path"] == nat.CBMM_MFMA, where
                                    for f in ("splits", "rps", "col_tiles", "row_tiles", "workspace"):
                                        assert p[f] == b[f], (f, where)
                                    assert (p["col_tiles"], p["row_tiles"]) == (u["col_tiles"], u["row_tiles"]), where   # the tiled path's counts
                                    assert p["rps"] % 32 == 0 and all(lo % 32 == 0 for lo, _ in gp.split_ranges(p, kdim)), where
                                    assert (p["tables"], p["copies"]) == (1, 32), where
                                    continue
                                for f in SHARED_WITH_PACKED:
                                    assert p[f] == u[f], (f, where)
                                if p["path"] == nat.CBMM_STREAM:
                                    assert (p["tables"], p["copies"]) == (4, 32), where
                                    assert p["lds"] == (4 * p["entries"] * 32 + p["mt"] * p["cols"] * 64) * 4, where
                                else:
                                    assert p["path"] == nat.CBMM_TILED and (p["tables"], p["copies"]) == (2, 1), where
                                    assert p["lds"] == u["lds"] + p["entries"] * 4, where
                            assert p["splits"] >= last_splits, (dt, bits, m, kdim, ncols, cus)   # the splits never shrink with more CUs
                            last_splits = p["splits"]


def _plans(lib, cus):
    return [(c, dtype, gplan(lib, gp.DT_CODE[dtype], c["m"], c["kdim"], c["ncols"], c["bits"], c["k"], c["group_rows"], cus)) for c in CASES for dtype in DTYPES]


@pytest.mark.parametrize("cus", CU_COUNTS)
def test_the_cases_hit_every_regime_and_walk_through_groups_in_every_way(lib, cus):
    hit, walks = set(), {}
    for c, dtype, p in _plans(lib, cus):
        r = gp.regime_of(c, p, dtype)
        hit.add(r)
        walks.setdefault(r[0], set()).update(gp.walks_of(c, p))
    assert hit == gp.required_regimes(), sorted(gp.required_regimes() - hit)
    for kernel in ("stream", "tiled", "mfma"):
        assert gp.required_walks(kernel) <= walks[kernel], (kernel, walks[kernel])
    assert any(c["kdim"] % c["group_rows"] and c["kdim"] > c["group_rows"] for c in CASES)      # a short last group
    assert any(c["kdim"] < c["group_rows"] for c in CASES)
    assert any(grouped_ref.groups_of(c) == 1 and c["kdim"] > 32 for c in CASES)                 # group_rows >= kdim
    assert {c["k"] for c in CASES} == {3, 4, 5, 16} and all(c["bits"] == (2 if c["k"] <= 4 else 4) for c in CASES)


def test_the_plans_the_case_list_was_written_for(lib):
    p = gplan(lib, nat.DT_F32, 1, 112, 70, 2, 3, 32, 256)
    assert (p["path"], p["splits"], p["rps"]) == (nat.CBMM_STREAM, 3, 38), p         # splits that start at rows 38 and 76, inside groups 1 and 2
    p = gplan(lib, nat.DT_F32, 17, 300, 50, 4, 16, 32, 256)
    assert (p["path"], p["splits"], p["rps"]) == (nat.CBMM_TILED, 2, 150), p         # the step of rows 158..165 lies across row 160
    p = gplan(lib, nat.DT_BF16, 17, 300, 50, 4, 16, 32, 256)
    assert (p["path"], p["splits"], p["rps"]) == (nat.CBMM_MFMA, 4, 96), p
    p = gplan(lib, nat.DT_F16, 17, 160, 130, 2, 3, 32, 256)
    assert (p["path"], p["splits"], p["rps"], p["max_groups_per_split"]) == (nat.CBMM_MFMA, 2, 96, 3), p


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[gp.case_id(c) for c in CASES])
def test_exact_data_is_exact_and_packs(ci):
    """Every partial sum of the exact data is exact in float32 in any order for the three activation types, and its labels fit the
    case's width: the packed buffer unpacks to them."""
    c = CASES[ci]
    lab, x, cen, bias = grouped_ref.exact_data(c, 9000 + ci)
    for dtype in DTYPES:
        cbmm_ref.assert_exact(x, grouped_ref.weights(cen, lab, c["kdim"], c["ncols"], c["group_rows"], dtype), bias)
    buf = packed_ref.pack(lab, c["kdim"], c["ncols"], c["bits"])
    assert buf.size == c["kdim"] * packed_ref.row_bytes(c["ncols"], c["bits"])
    assert np.array_equal(packed_ref.unpack(buf, c["kdim"], c["ncols"], c["bits"]), lab.astype(np.uint8))


def test_argument_errors_come_back_before_any_hip_call(lib):
    out = (ctypes.c_int64 * nat.CBPK_GROUPED_PLAN_LEN)()
    ok = dict(dt=nat.DT_F32, m=4, kdim=112, ncols=70, bits=4, k=16, rows=32, cus=256)

    def plan_rc(**kw):
        a = dict(ok, **kw)
        return lib.nnc_cbpk_grouped_plan(a["dt"], a["m"], a["kdim"], a["ncols"], a["bits"], a["k"], a["rows"], a["cus"], a.get("out", out))

    assert plan_rc() == 0
    for rows in (0, -32, 1, 16, 31, 33, 48, 100, (1 << 41)):
        assert plan_rc(rows=rows) == NNC_EINVAL, rows
        assert b"group_rows" in lib.nnc_last_error() or rows > (1 << 40)
    for bits in (0, 1, 3, 8, -4):
        assert plan_rc(bits=bits, k=1) == NNC_EINVAL, bits
    for bits, k in ((4, 0), (4, -1), (4, 17), (2, 5), (2, 16), (4, 256)):
        assert plan_rc(bits=bits, k=k) == NNC_EINVAL, (bits, k)
    for bad in (dict(dt=3), dict(dt=-1), dict(m=-1), dict(kdim=-1), dict(ncols=-1), dict(cus=0), dict(out=None), dict(m=(1 << 41))):
        assert plan_rc(**bad) == NNC_EINVAL, bad

    # the call itself: host pointers that are never dereferenced (every one of these returns before a HIP call)
    buf = (ctypes.c_float * 64)()
    a = (ctypes.addressof(buf) + 15) & ~15
    pb = lambda kdim, ncols, bits: lib.nnc_cbpk_pack_bytes(kdim, ncols, bits)   # noqa: E731

    def call_rc(x=a, dt=nat.DT_F32, m=4, kdim=112, packed=a, pbytes=None, bits=4, ncols=70, centers=a, k=16, rows=32, y=a, ydt=nat.DT_F32, ws=a,
                ws_bytes=1 << 30):
        pbytes = pb(kdim, ncols, bits) if pbytes is None else pbytes
        return lib.nnc_cbpk_grouped(x, dt, m, kdim, packed, pbytes, bits, ncols, centers, k, rows, None, 0, y, ydt, ws, ws_bytes, None)

    assert pb(112, 70, 4) == 112 * 48
    for bad in (dict(rows=0), dict(rows=31), dict(rows=48), dict(rows=-64), dict(k=0), dict(k=17), dict(bits=2, k=5), dict(bits=3, pbytes=112 * 48),
                dict(bits=8, pbytes=112 * 80), dict(dt=7), dict(m=-1), dict(kdim=-2, pbytes=0), dict(ncols=-3, pbytes=0),
                dict(pbytes=112 * 48 - 1), dict(pbytes=112 * 48 + 16), dict(pbytes=112 * 70), dict(packed=a + 4), dict(packed=a + 8), dict(packed=None),
                dict(centers=None), dict(y=None), dict(x=None), dict(ws_bytes=-1),
                dict(ydt=nat.DT_BF16), dict(dt=nat.DT_BF16, ydt=nat.DT_F16), dict(dt=nat.DT_F16, ydt=nat.DT_BF16), dict(ydt=9),
                dict(x=a + 2), dict(y=a + 2), dict(dt=nat.DT_BF16, x=a + 1), dict(dt=nat.DT_F16, ydt=nat.DT_F16, y=a + 1)):
        assert call_rc(**bad) == NNC_EINVAL, bad
    need = lib.nnc_cbpk_grouped_workspace_bytes(nat.DT_F32, 1, 4096, 64, 4)
    assert need > 0 and need == lib.nnc_cbpk_workspace_bytes(1, 4096, 64, 4)
    assert call_rc(m=1, kdim=4096, ncols=64, ws_bytes=need - 4) == NNC_ENOSPACE
    assert call_rc(m=1, kdim=4096, ncols=64, ws=None, ws_bytes=need) == NNC_EINVAL
    assert call_rc(m=0) == 0 and call_rc(ncols=0, pbytes=0) == 0          # no-ops: nothing is launched
    assert lib.nnc_cbpk_grouped_workspace_bytes(nat.DT_F32, -1, 5, 5, 4) == 0
    assert lib.nnc_cbpk_grouped_workspace_bytes(nat.DT_F32, 4, 5, 5, 3) == 0


def test_ops_argument_errors_need_no_device():
    torch = pytest.importorskip("torch")
    from neural_network_compression_amd import ops

    with pytest.raises(TypeError):
        ops.cbpk_grouped_plan(torch.float64, 4, 112, 70, 4, 16, 32, 256)
    with pytest.raises(nat.NncError):
        ops.cbpk_grouped_plan(torch.float32, 4, 112, 70, 4, 16, 48, 256)
    with pytest.raises(nat.NncError):
        ops.cbpk_grouped_plan(torch.bfloat16, 4, 112, 70, 4, 17, 32, 256)
    with pytest.raises(TypeError):                                  # a tensor on the host
        ops.grouped_packed_codebook_matmul(torch.zeros(4, 112), None, torch.zeros(4, 16), 32)
    p = ops.cbpk_grouped_plan(torch.float16, 17, 160, 130, 2, 3, 32, 256)
    assert (p["groups"], p["group_rows"], p["max_groups_per_split"], p["path"], p["tables"]) == (5, 32, 3, nat.CBMM_MFMA, 1)
    from neural_network_compression_amd import compressed

    with pytest.raises(ValueError, match="packed"):
        compressed.pack_grouped_layers(torch.nn.Identity(), packed=False)
