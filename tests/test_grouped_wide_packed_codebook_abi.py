"""CPU checks of the C ABI of the group-wise codebook layer on 5- and 6-bit split-plane indices (include/nnc_cbwp_grouped.h, DESIGN.md
section 38): the header against the bound signatures, the invariants of the plan and the argument errors.  No device needed."""
import ctypes
import os
import re

import pytest
import torch

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from neural_network_compression_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"nnc_cbwp_grouped", "nnc_cbwp_grouped_plan", "nnc_cbwp_grouped_workspace_bytes"}
STREAM, TILED, MFMA = nat.CBMM_STREAM, nat.CBMM_TILED, nat.CBMM_MFMA


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_symbols_header_and_signatures_agree(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nnc_cbwp_grouped.h")).read(), flags=re.S)
    protos = re.findall(r"\b(int64_t|int)\s+(nnc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    assert {p[1] for p in protos} == set(nat.GROUPED_WIDE_PACKED_SIGNATURES) == NAMES and len(protos) == len(NAMES)
    for other in (nat.SIGNATURES, nat.WIDE_PACKED_SIGNATURES, nat.WIDE_PACKED_GRAD_SIGNATURES):
        assert not NAMES & set(other)
    raw = ctypes.CDLL(nat.lib_path())
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "int32_t": ctypes.c_int32}
    for ret, name, args in protos:
        res, argtypes = nat.GROUPED_WIDE_PACKED_SIGNATURES[name]
        assert hasattr(raw, name) and res is ctype[ret]
        decl = [a.strip() for a in args.split(",")]
        assert len(decl) == len(argtypes), name
        for d, a in zip(decl, argtypes):
            assert (a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64))) if "*" in d else (a is ctype[d.split()[0]]), (name, d)
    assert os.path.join(nbuild.CSRC, "nnc_cbwp_grouped.hip") in nbuild.SOURCES
    assert os.path.join(nbuild.INCLUDE, "nnc_cbwp_grouped.h") in nbuild._headers()
    plan_len = int(re.search(r"#define NNC_CBWP_GROUPED_PLAN_LEN (\d+)", text).group(1))
    assert len(nat.CBWP_GROUPED_PLAN_FIELDS) == plan_len == nat.CBWP_GROUPED_PLAN_LEN


@pytest.mark.parametrize("cus", [80, 256, 304])
@pytest.mark.parametrize("bits,k", [(5, 17), (6, 64)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_plan_invariants(lib, dtype, bits, k, cus):
    for m in (1, 16, 17, 130, 4096):
        for kdim, ncols in ((33, 129), (200, 300), (2048, 127), (4096, 4096)):
            for group_rows in (32, 96, 4096):
                p = ops.cbwp_grouped_plan(dtype, m, kdim, ncols, bits, k, group_rows, cus)
                path = STREAM if m <= 16 else TILED if dtype is torch.float32 else MFMA
                assert p["path"] == path and p["group_rows"] == group_rows and p["groups"] == -(-kdim // group_rows)
                assert p["tables"] == {STREAM: 4, TILED: 2, MFMA: 1}[path] and 0 < p["lds"] <= 64 * 1024
                assert 1 <= p["max_groups_per_split"] <= p["groups"]
                if path == MFMA:
                    assert p["rps"] % 32 == 0
                else:
                    u = ops.cbwp_plan(dtype, m, kdim, ncols, bits, k, cus)
                    assert all(p[f] == u[f] for f in ("path", "vb", "mt", "splits", "rps"))
                assert p["workspace"] == lib.nnc_cbwp_grouped_workspace_bytes(p["dtype"], m, kdim, ncols, bits) or cus != 256


def test_argument_errors_come_back_without_a_device(lib):
    out = (ctypes.c_int64 * nat.CBWP_GROUPED_PLAN_LEN)()
    for args, msg in (((0, 4, 64, 16, 5, 16, 32, 256, out), "k <= 16"), ((0, 4, 64, 16, 6, 65, 32, 256, out), "k > 64"),
                      ((0, 4, 64, 16, 9, 64, 32, 256, out), "9 bits would be larger"), ((0, 4, 64, 16, 5, 17, 48, 256, out), "multiple of 32")):
        assert lib.nnc_cbwp_grouped_plan(*args) == -1 and msg in lib.nnc_last_error().decode()
    P = 0x1000
    nb = lib.nnc_cbwp_pack_bytes(64, 16, 5)
    assert lib.nnc_cbwp_grouped(P, 0, 4, 64, P + 8, nb, 5, 16, P, 17, 32, None, 0, P, 0, None, 0, None) == -1
    assert "16-byte aligned" in lib.nnc_last_error().decode()
    assert lib.nnc_cbwp_grouped(P, 0, 4, 64, P, nb - 1, 5, 16, P, 17, 32, None, 0, P, 0, None, 0, None) == -1
    assert "packed_bytes" in lib.nnc_last_error().decode()
    with pytest.raises(TypeError, match="CUDA"):
        ops.grouped_wide_packed_codebook_matmul(torch.zeros(3, 64), None, torch.zeros(2, 17), 32)
