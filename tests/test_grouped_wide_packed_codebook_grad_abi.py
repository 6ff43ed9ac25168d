"""CPU checks of the C ABI of the backward pass of the group-wise codebook layer on 5- and 6-bit split-plane indices
(include/nnc_cbwpgrad_grouped.h): the header against the bound signatures, the argument errors and the
invariants of the two plans.  No device needed."""
import ctypes
import os
import re

import pytest
import torch

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from neural_network_compression_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM, TILED, MFMA = nat.CBMM_STREAM, nat.CBMM_TILED, nat.CBMM_MFMA
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
WIDTHS = [(5, 17), (5, 32), (6, 33), (6, 64)]
TAIL = ("group_rows", "groups", "rows_per_group", "max_groups_per_workgroup", "held")
BASE4_CASES = {(16, 1), (8, 1), (4, 1), (16, 2), (8, 2), (4, 2), (8, 4), (4, 4), (4, 8), (2, 16)}   # (VB, MT): WPG_BASE4_CASES


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_symbols_header_and_signatures_agree(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nnc_cbwpgrad_grouped.h")).read(), flags=re.S)
    protos = re.findall(r"\b(int64_t|int)\s+(nnc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    mine = nat.GROUPED_WIDE_PACKED_GRAD_SIGNATURES
    assert {p[1] for p in protos} == set(mine) and len(protos) == 6
    others = [v for n, v in vars(nat).items() if n.endswith("SIGNATURES") and v is not mine]
    assert len(others) >= 15 and not any(set(mine) & set(o) for o in others)
    raw = ctypes.CDLL(nat.lib_path())
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "int32_t": ctypes.c_int32}
    for ret, name, args in protos:
        res, argtypes = mine[name]
        assert hasattr(raw, name) and res is ctype[ret] and getattr(lib, name).argtypes == argtypes
        decl = [a.strip() for a in args.split(",")]
        assert len(decl) == len(argtypes), name
        for d, a in zip(decl, argtypes):
            assert (a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64))) if "*" in d else (a is ctype[d.split()[0]]), (name, d)
    assert os.path.join(nbuild.CSRC, "nnc_cbwpgrad_grouped.hip") in nbuild.SOURCES
    assert os.path.join(nbuild.INCLUDE, "nnc_cbwpgrad_grouped.h") in nbuild._headers()
    assert nat.CBWPDX_GROUPED_PLAN_FIELDS[-5:] == nat.CBWPDC_GROUPED_PLAN_FIELDS[-5:] == TAIL
    assert len(nat.CBWPDX_GROUPED_PLAN_FIELDS) == int(re.search(r"#define NNC_CBWPGRAD_GROUPED_PLAN_LEN (\d+)", text).group(1))
    assert [f.upper() for f in TAIL] == [n for n, _ in sorted(re.findall(r"#define NNC_CBWPGRAD_GROUPED_P_(\w+) (\d+)", text), key=lambda t: int(t[1]))]


def test_argument_errors_come_back_without_a_device(lib):
    out = (ctypes.c_int64 * len(nat.CBWPDX_GROUPED_PLAN_FIELDS))()
    for plan in (lib.nnc_cbwp_grouped_dx_plan, lib.nnc_cbwp_grouped_dc_plan):
        for args, msg in (((0, 4, 8, 16, 9, 257, 32, 256, out), "k > 64 (bits 9) is refused"), ((0, 4, 8, 16, 6, 65, 32, 256, out), "k > 64"),
                          ((0, 4, 8, 16, 4, 17, 32, 256, out), "bits must be 5 or 6"), ((0, 4, 8, 16, 5, 16, 32, 256, out), "k <= 16 is refused"),
                          ((0, 4, 8, 16, 5, 33, 32, 256, out), "k outside 1..2^bits"), ((3, 4, 8, 16, 5, 17, 32, 256, out), "x_dtype"),
                          ((0, 4, 8, 16, 5, 17, 48, 256, out), "group_rows must be a positive multiple of 32"),
                          ((0, 4, 1 << 40, 1, 6, 64, 32, 256, out), "more than 2^30 bins"), ((0, 1 << 30, 1 << 30, 1, 5, 17, 32, 256, out), "size too large"),
                          ((0, 4, 8, 16, 5, 17, 32, 0, out), "cus < 1"), ((0, -1, 8, 16, 5, 17, 32, 256, out), "negative size"),
                          ((0, 4, 8, 16, 5, 17, 32, 256, None), "out is NULL")):
            assert plan(*args) == -1 and msg in lib.nnc_last_error().decode(), msg
    P, nb = 0x1000, lib.nnc_cbwp_pack_bytes(8, 16, 5)
    err = lambda: lib.nnc_last_error().decode()                                                   # noqa: E731
    dx, dc = lib.nnc_cbwp_grouped_dx, lib.nnc_cbwp_grouped_dc
    assert dx(P, 0, 4, 8, P, nb - 1, 5, 16, P, 17, 32, P, 0, None, 0, None) == -1 and "packed_bytes" in err()
    assert dx(P, 0, 4, 8, P + 8, nb, 5, 16, P, 17, 32, P, 0, None, 0, None) == -1 and "16-byte aligned" in err()
    assert dx(P, 0, 4, 8, P, nb, 5, 16, P, 17, 32, P, 1, None, 0, None) == -1 and "dx_dtype" in err()
    assert dx(P + 1, 1, 4, 8, P, nb, 5, 16, P, 17, 32, P, 1, None, 0, None) == -1 and "not aligned" in err()
    assert dx(P, 0, 4, 8, P, nb, 5, 16, None, 17, 32, P, 0, None, 0, None) == -1 and "centers is NULL" in err()
    assert dx(P, 0, 4, 8, P, nb, 5, 16, P, 17, 32, None, 0, None, 0, None) == -1 and "dx is NULL" in err()
    assert dx(P, 0, 4, 8, P, nb, 5, 16, P, 17, 40, P, 0, None, 0, None) == -1 and "group_rows" in err()
    assert dc(P, P + 1, 2, 4, 8, P, nb, 5, 16, 17, 32, P, 1, P, 1 << 20, None) == -1 and "not aligned" in err()
    assert dc(P, P, 0, 4, 8, P, nb, 5, 16, 17, 32, None, 1, P, 1 << 20, None) == -1 and "dc is NULL" in err()
    assert dc(P, None, 0, 4, 8, P, nb, 5, 16, 17, 32, P, 1, P, 1 << 20, None) == -1 and "x or g is NULL" in err()
    assert dc(P, P, 0, 4, 8, P, nb, 5, 16, 17, 32, P, 1, P + 4, 1 << 20, None) == -1 and "8-byte aligned" in err()
    assert dc(P, P, 0, 4, 8, P, nb, 5, 16, 17, 32, P, 1, P, 8, None) == -2 and "workspace" in err()          # NNC_ENOSPACE
    nb = lib.nnc_cbwp_pack_bytes(200, 1100, 5)
    assert dx(P, 0, 16, 200, P, nb, 5, 1100, P, 17, 32, P, 0, P, 8, None) == -2 and "workspace" in err()
    for fn in (ops.grouped_wide_packed_codebook_matmul_dx, ops.grouped_wide_packed_codebook_linear):
        with pytest.raises(TypeError, match="CUDA|WidePackedCodes"):
            fn(torch.zeros(3, 16), None, torch.zeros(1, 17), 32)
    with pytest.raises(TypeError, match="cbwp|dtype"):
        ops.cbwp_grouped_dx_plan(torch.int8, 4, 8, 16, 5, 17, 32, 256)


@pytest.mark.parametrize("cus", [1, 8, 104, 256, 304])
@pytest.mark.parametrize("bits,k", WIDTHS)
def test_plan_invariants(lib, bits, k, cus):
    seen = set()
    for dtype in DTYPES:
        for m in (1, 3, 16, 17, 130, 4096):
            for kdim, ncols in ((1, 1), (33, 129), (200, 300), (200, 1100), (2048, 127), (4096, 4096), (5000, 5000), (64, 100000)):
                for group_rows in (32, 96, 128, 8192):
                    dx, dc = (f(dtype, m, kdim, ncols, bits, k, group_rows, cus) for f in (ops.cbwp_grouped_dx_plan, ops.cbwp_grouped_dc_plan))
                    flat = (ops.cbwp_dx_plan(dtype, m, kdim, ncols, bits, k, cus), ops.cbwp_dc_plan(dtype, m, kdim, ncols, bits, k, cus))
                    groups = -(-kdim // group_rows)
                    in_tile = 1 if group_rows % 128 == 0 else (4 if group_rows == 32 else 2)
                    for p, u, own in ((dx, flat[0], ("lds", "copies")), (dc, flat[1], ("copies", "workspace"))):
                        assert {f: v for f, v in p.items() if f not in own + TAIL} == {f: v for f, v in u.items() if f not in own}
                        assert (p["group_rows"], p["groups"]) == (group_rows, groups) and 0 < p["lds"] <= 64 * 1024
                        assert 1 <= p["max_groups_per_workgroup"] <= groups
                        if m <= 16:
                            seen.add((p["vb"], p["mt"]))
                            assert p["rows_per_group"] * (p["row_tiles"] - 1) < kdim <= p["rows_per_group"] * p["row_tiles"]
                        else:
                            assert p["rows_per_group"] == 0 and p["held"] == in_tile and p["max_groups_per_workgroup"] <= in_tile
                            assert p["copies"] * (p["held"] if p is dc or dtype is not torch.float32 else 1) == u["copies"]
                    if m <= 16:   # a table per wave and no staging row; one set of bins, the ungrouped kernel's
                        assert (dx["held"], dx["lds"], dx["copies"]) == (4, 4 * (1 << bits) * 32 * 4, 32)
                        assert (dc["held"], dc["lds"], dc["copies"]) == (1, flat[1]["lds"], 32)
                    elif dtype is torch.float32:
                        assert dx["lds"] == flat[0]["lds"] + (in_tile - 1) * (1 << bits) * 4 and dc["lds"] == flat[1]["lds"]
                    else:
                        assert dx["lds"] == flat[0]["lds"] and dc["lds"] == flat[1]["lds"]
                    if cus == 256:
                        assert dx["workspace"] == lib.nnc_cbwp_grouped_dx_workspace_bytes(dx["dtype"], m, kdim, ncols, bits)
                        assert dc["workspace"] == lib.nnc_cbwp_grouped_dc_workspace_bytes(dc["dtype"], m, kdim, ncols, bits, k, group_rows) == 64 + 8 * groups * k
    assert seen and seen <= BASE4_CASES   # and every plan above found its instantiation: a plan without one is NNC_EINVAL


@pytest.mark.parametrize("bits,k", WIDTHS)
def test_the_empty_shapes_launch_nothing(lib, bits, k):
    for dtype in DTYPES:
        dxp, dcp = ops.cbwp_grouped_dx_plan, ops.cbwp_grouped_dc_plan
        assert dxp(dtype, 0, 8, 16, bits, k, 32, 256)["path"] == dxp(dtype, 4, 0, 16, bits, k, 32, 256)["path"] == nat.CBMM_NONE
        assert dxp(dtype, 20, 8, 0, bits, k, 32, 256)["path"] == nat.CBMM_ZERO
        assert {dcp(dtype, *s, bits, k, 32, 256)["path"] for s in ((0, 8, 16), (4, 0, 16), (20, 8, 0))} == {nat.CBMM_ZERO}
        assert lib.nnc_cbwp_grouped_dc_workspace_bytes(ops._X_DT[dtype], 4, 0, 16, bits, k, 32) == 0
