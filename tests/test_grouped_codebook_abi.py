"""CPU checks of the group-wise codebook matmul's C ABI (include/nnc.h, nnc_cbmm_grouped*): the plan is the
ungrouped one plus three fields, the case list of the GPU suite (tests/helpers/grouped_ref.py) reaches every kernel and every way
of walking through groups, its exact data is exact, and every argument error comes back before any HIP call, so none of this
needs a device."""
import ctypes
import os
import re

import numpy as np
import pytest

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from tests.helpers import cbmm_ref, grouped_ref
from tests.helpers.grouped_ref import CASES, CU_COUNTS, DTYPES

NNC_EINVAL, NNC_ENOSPACE = -1, -2
SAME_AS_UNGROUPED = ("path", "vb", "mt", "col_tiles", "row_tiles", "splits", "rps")


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def gplan(lib, dt, m, kdim, ncols, k, group_rows, cus, addr=0):
    out = (ctypes.c_int64 * nat.CBMM_GROUPED_PLAN_LEN)()
    rc = lib.nnc_cbmm_grouped_plan(dt, m, kdim, ncols, k, group_rows, cus, addr, out)
    assert rc == 0, (dt, m, kdim, ncols, k, group_rows, cus, addr, lib.nnc_last_error())
    return dict(zip(nat.CBMM_GROUPED_PLAN_FIELDS, out))


def uplan(lib, dt, m, kdim, ncols, k, cus, addr=0):
    """The ungrouped plan for the same call: nnc_cbmm_plan for float32 x, nnc_cbmm_h16_plan for half x, label_bytes 1."""
    if dt == nat.DT_F32:
        out = (ctypes.c_int64 * nat.CBMM_PLAN_LEN)()
        assert lib.nnc_cbmm_plan(m, kdim, ncols, 1, k, cus, addr, out) == 0
        return dict(zip(nat.CBMM_PLAN_FIELDS, out))
    out = (ctypes.c_int64 * nat.CBMM_H16_PLAN_LEN)()
    assert lib.nnc_cbmm_h16_plan(dt, m, kdim, ncols, 1, k, cus, addr, out) == 0
    return dict(zip(nat.CBMM_H16_PLAN_FIELDS, out))


def test_symbols_header_and_signatures_agree(lib):
    raw = ctypes.CDLL(nat.lib_path())
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nnc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nnc_cbmm_grouped\w*)\s*\(", code))
    assert declared == {"nnc_cbmm_grouped", "nnc_cbmm_grouped_workspace_bytes", "nnc_cbmm_grouped_plan"}
    for s in declared:
        assert hasattr(raw, s) and s in nat.SIGNATURES, s
    defs = {k: int(v) for k, v in re.findall(r"#define (NNC_\w+) (\d+)", text)}
    assert defs["NNC_CBMM_GROUPED_PLAN_LEN"] == nat.CBMM_GROUPED_PLAN_LEN == len(nat.CBMM_GROUPED_PLAN_FIELDS)
    for name in ("group_rows", "groups", "max_groups_per_split"):
        assert defs["NNC_CBMM_GROUPED_P_" + name.upper()] == nat.CBMM_GROUPED_PLAN_FIELDS.index(name)
    assert nat.CBMM_GROUPED_PLAN_FIELDS[: nat.CBMM_H16_PLAN_LEN] == nat.CBMM_H16_PLAN_FIELDS
    assert grouped_ref.DT_CODE == {"f32": nat.DT_F32, "bf16": nat.DT_BF16, "fp16": nat.DT_F16}
    assert (grouped_ref.PATH_STREAM, grouped_ref.PATH_TILED, grouped_ref.PATH_MFMA) == (nat.CBMM_STREAM, nat.CBMM_TILED, nat.CBMM_MFMA)


PLAN_MS = [0, 1, 2, 3, 8, 16, 17, 128, 129, 4096]
PLAN_KDIMS = [0, 1, 31, 32, 33, 112, 160, 300, 1001, 4096]
PLAN_NCOLS = [0, 1, 50, 64, 130, 4096]
PLAN_ROWS = [32, 128, 1 << 20]


def test_plan_is_the_ungrouped_plan_plus_three_fields(lib):
    for dt in (nat.DT_F32, nat.DT_BF16, nat.DT_F16):
        for m in PLAN_MS:
            for kdim in PLAN_KDIMS:
                for ncols in PLAN_NCOLS:
                    ws = lib.nnc_cbmm_grouped_workspace_bytes(dt, m, kdim, ncols)
                    ungrouped_ws = (lib.nnc_cbmm_workspace_bytes if dt == nat.DT_F32 else lib.nnc_cbmm_h16_workspace_bytes)(m, kdim, ncols, 1)
                    assert ws == ungrouped_ws
                    for cus in CU_COUNTS:
                        for k in ((16,) if cus != 256 else (3, 256)):
                            u = uplan(lib, dt, m, kdim, ncols, k, cus)
                            for rows in PLAN_ROWS:
                                p = gplan(lib, dt, m, kdim, ncols, k, rows, cus)
                                where = (dt, m, kdim, ncols, k, rows, cus, p, u)
                                for f in SAME_AS_UNGROUPED:
                                    assert p[f] == u[f], (f, where)
                                assert p["workspace"] == u["workspace"] <= ws, where
                                assert p["dtype"] == dt and p["group_rows"] == rows, where
                                assert p["groups"] == -(-kdim // rows), where
                                assert p["lds"] <= 64 * 1024, where
                                if p["path"] in (nat.CBMM_NONE, nat.CBMM_BIAS):
                                    assert p["max_groups_per_split"] == 0, where
                                    continue
                                spans = [(hi - 1) // rows - lo // rows + 1 for lo, hi in grouped_ref.split_ranges(p, kdim)]
                                assert p["max_groups_per_split"] == max(spans) >= 1, where
                                assert p["max_groups_per_split"] <= p["groups"], where
                                if p["path"] == nat.CBMM_MFMA:
                                    assert p["rps"] % 32 == 0, where     # a k step of 32 never lies across a boundary
                                if p["path"] == nat.CBMM_TILED:
                                    assert p["copies"] == 2 and p["lds"] == u["lds"] + (k + 1) * 4, where
                                else:
                                    assert p["lds"] == u["lds"] and p["entries"] == 256, where


def test_plan_follows_the_label_address(lib):
    for addr in (0, 4096, 4097, 4100, 4104):
        for ncols in (64, 70):
            p, u = gplan(lib, nat.DT_F32, 4, 112, ncols, 16, 32, 256, addr), uplan(lib, nat.DT_F32, 4, 112, ncols, 16, 256, addr)
            assert p["aligned"] == u["aligned"] == int(addr % 16 == 0 and ncols % 16 == 0)


def _plans(lib, cus):
    return [(c, dtype, gplan(lib, grouped_ref.DT_CODE[dtype], c["m"], c["kdim"], c["ncols"], c["k"], c["group_rows"], cus, 4096 + c["off"]))
            for c in CASES for dtype in DTYPES]


@pytest.mark.parametrize("cus", [64, 256, 1024])
def test_the_cases_hit_every_regime(lib, cus):
    hit = {grouped_ref.regime_of(p, dtype) for _, dtype, p in _plans(lib, cus)}
    assert hit == grouped_ref.required_regimes(), sorted(grouped_ref.required_regimes() - hit)


@pytest.mark.parametrize("cus", [64, 256, 1024])
def test_the_cases_walk_through_groups_in_every_way(lib, cus):
    """Per kernel: a split through three groups or more and a split that starts inside a group (the MFMA tile's splits start on k
    steps of 32, so only on a boundary or, with group_rows 64, in the middle of a group); and, over the list, a short last group,
    kdim < group_rows, one group, K in {3, 16, 256}, aligned and unaligned label rows."""
    seen = {}
    for c, dtype, p in _plans(lib, cus):
        kernel = grouped_ref.regime_of(p, dtype)[0]
        s = seen.setdefault(kernel, set())
        rows = c["group_rows"]
        if p["max_groups_per_split"] >= 3:
            s.add("three groups in a split")
        if p["splits"] > 1 and any(lo % rows for lo, _ in grouped_ref.split_ranges(p, c["kdim"])):
            s.add("a split starts inside a group")
        if kernel == "tiled" and any(lo // rows != (min(lo + 8, hi) - 1) // rows for lo0, hi in grouped_ref.split_ranges(p, c["kdim"])
                                     for lo in range(lo0, hi, 8)):
            s.add("a TB_K step across a boundary")
        if kernel == "stream" and p["groups"] > 1:
            s.add("aligned" if p["aligned"] else "unaligned")
    for kernel in ("stream", "tiled", "mfma"):
        want = {"three groups in a split", "a split starts inside a group"}
        want |= {"a TB_K step across a boundary"} if kernel == "tiled" else set()
        want |= {"aligned", "unaligned"} if kernel == "stream" else set()
        assert want <= seen[kernel], (kernel, want - seen[kernel])
    assert any(c["kdim"] % c["group_rows"] and c["kdim"] > c["group_rows"] for c in CASES)      # a short last group
    assert any(c["kdim"] < c["group_rows"] for c in CASES)
    assert any(grouped_ref.groups_of(c) == 1 and c["kdim"] > 32 for c in CASES)                 # group_rows >= kdim
    assert {c["k"] for c in CASES} == {3, 16, 256}


@pytest.mark.parametrize("ci", range(len(CASES)), ids=[grouped_ref.case_id(c) for c in CASES])
def test_exact_data_is_exact(ci):
    """Every partial sum of the exact data is exact in float32 in any order, with the centres as they are (float32 x) and rounded
    to bf16 / fp16; the offsets tell the groups apart after the rounding too."""
    c = CASES[ci]
    lab, x, cen, bias = grouped_ref.exact_data(c, 7000 + ci)
    for dtype in DTYPES:
        w = grouped_ref.weights(cen, lab, c["kdim"], c["ncols"], c["group_rows"], dtype)
        cbmm_ref.assert_exact(x, w, bias)
        assert cbmm_ref.exact_grid_bits(w) <= 2
        r = grouped_ref.round_centres(cen, dtype)
        if r.shape[0] > 1:
            assert np.all(r[1:].min(axis=1) - r[:-1].max(axis=1) >= 48), dtype


def test_weights_reference_reads_the_group_of_the_row():
    cen = np.array([[1.0, 2.0], [10.0, 20.0], [100.0, 200.0]], dtype=np.float32)
    lab = np.zeros((70, 3), dtype=np.int64)
    lab[:, 1], lab[:, 2] = 1, 2                     # column 2: an index >= K
    w = grouped_ref.weights(cen, lab, 70, 3, 32)
    assert np.array_equal(w[[0, 31, 32, 63, 64, 69]], np.array([[1, 2, 0], [1, 2, 0], [10, 20, 0], [10, 20, 0], [100, 200, 0], [100, 200, 0]], dtype=np.float32))


def test_argument_errors_come_back_before_any_hip_call(lib):
    out = (ctypes.c_int64 * nat.CBMM_GROUPED_PLAN_LEN)()
    ok = dict(dt=nat.DT_F32, m=4, kdim=112, ncols=70, k=16, rows=32, cus=256)

    def plan_rc(**kw):
        a = dict(ok, **kw)
        return lib.nnc_cbmm_grouped_plan(a["dt"], a["m"], a["kdim"], a["ncols"], a["k"], a["rows"], a["cus"], 0, a.get("out", out))

    assert plan_rc() == 0
    for rows in (0, -32, 1, 16, 31, 33, 48, 100, (1 << 41)):
        assert plan_rc(rows=rows) == NNC_EINVAL, rows
        assert b"group_rows" in lib.nnc_last_error() or rows > (1 << 40)
    for k in (0, -1, 257, 300, 65536):               # k > 256 would need two-byte labels: there is no such form
        assert plan_rc(k=k) == NNC_EINVAL, k
    assert b"uint8" in lib.nnc_last_error()
    for bad in (dict(dt=3), dict(dt=-1), dict(m=-1), dict(kdim=-1), dict(ncols=-1), dict(cus=0), dict(out=None), dict(m=(1 << 41))):
        assert plan_rc(**bad) == NNC_EINVAL, bad

    # the call itself: host pointers that are never dereferenced (every one of these returns before a HIP call)
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)

    def call_rc(x=a, dt=nat.DT_F32, m=4, kdim=112, labels=a, ncols=70, centers=a, k=16, rows=32, y=a, ydt=nat.DT_F32, ws=a, ws_bytes=1 << 30):
        return lib.nnc_cbmm_grouped(x, dt, m, kdim, labels, ncols, centers, k, rows, None, 0, y, ydt, ws, ws_bytes, None)

    for bad in (dict(rows=0), dict(rows=48), dict(rows=-64), dict(k=0), dict(k=257), dict(dt=7), dict(m=-1), dict(kdim=-2), dict(ncols=-3),
                dict(centers=None), dict(y=None), dict(x=None), dict(labels=None), dict(ws_bytes=-1),
                dict(ydt=nat.DT_BF16), dict(dt=nat.DT_BF16, ydt=nat.DT_F16), dict(dt=nat.DT_F16, ydt=nat.DT_BF16), dict(ydt=9),
                dict(x=a + 2), dict(y=a + 2), dict(dt=nat.DT_BF16, x=a + 1), dict(dt=nat.DT_F16, ydt=nat.DT_F16, y=a + 1)):
        assert call_rc(**bad) == NNC_EINVAL, bad
    need = lib.nnc_cbmm_grouped_workspace_bytes(nat.DT_F32, 1, 4096, 64)
    assert need > 0
    assert call_rc(m=1, kdim=4096, ncols=64, ws_bytes=need - 4) == NNC_ENOSPACE
    assert call_rc(m=1, kdim=4096, ncols=64, ws=None, ws_bytes=need) == NNC_EINVAL
    assert call_rc(m=0) == 0 and call_rc(ncols=0) == 0          # no-ops: nothing is launched
    assert lib.nnc_cbmm_grouped_workspace_bytes(nat.DT_F32, -1, 5, 5) == 0


def test_ops_argument_errors_need_no_device():
    torch = pytest.importorskip("torch")
    from neural_network_compression_amd import ops

    with pytest.raises(TypeError):
        ops.cbmm_grouped_plan(torch.float64, 4, 112, 70, 16, 32, 256)
    with pytest.raises(nat.NncError):
        ops.cbmm_grouped_plan(torch.float32, 4, 112, 70, 16, 48, 256)
    with pytest.raises(nat.NncError):
        ops.cbmm_grouped_plan(torch.bfloat16, 4, 112, 70, 257, 32, 256)
    with pytest.raises(TypeError):                                  # tensors on the host
        ops.grouped_codebook_matmul(torch.zeros(4, 112), torch.zeros(112 * 70, dtype=torch.uint8), torch.zeros(4, 16), 112, 70, 32)
    p = ops.cbmm_grouped_plan(torch.float16, 17, 160, 130, 16, 32, 256)
    assert (p["groups"], p["group_rows"], p["max_groups_per_split"], p["path"]) == (5, 32, 3, nat.CBMM_MFMA)


def test_fit_argument_errors_need_no_device():
    """get_quantized_weight_grouped's ValueErrors are raised before any fit, so before any device call."""
    from neural_network_compression_amd.common import utility

    kernel = np.zeros((112, 40), dtype=np.float32)
    for rows in (0, 16, 48, -32, 32.0):
        with pytest.raises(ValueError, match="group_rows"):
            utility.get_quantized_weight_grouped(kernel, rows, bits=4)
    with pytest.raises(ValueError, match="256"):
        utility.get_quantized_weight_grouped(kernel, 32, bits=9)
    with pytest.raises(ValueError, match="256"):
        utility.get_quantized_weight_grouped(kernel, 32, bits=8, mode="density", cdfs_by_group=[None] * 4)
    with pytest.raises(ValueError, match="2-D"):
        utility.get_quantized_weight_grouped(np.zeros((3, 3, 4, 8), dtype=np.float32), 32, bits=2)
    with pytest.raises(ValueError, match="fewer than"):               # the last group: 1 row of 40 weights < 2**6 + 1
        utility.get_quantized_weight_grouped(np.zeros((97, 40), dtype=np.float32), 32, bits=6)
    with pytest.raises(ValueError, match="cdfs_by_group"):
        utility.get_quantized_weight_grouped(kernel, 32, bits=2, mode="density", cdfs_by_group=[None] * 3)
    assert utility.grouped_slices((112, 40), 32, 4, "linear") == [(0, 32), (32, 64), (64, 96), (96, 112)]
    assert utility.grouped_slices((20, 40), 64, 4, "linear") == [(0, 20)]
