"""CPU checks of the C ABI of the 5-, 6- and 9-bit split-plane ("wide packed") codebook layer (include/nnc_cbwp.h, DESIGN.md section
36): the header against the bound signatures, the row formula, the width rule and the invariants of the plan.  No device needed."""
import ctypes
import os
import re

import pytest
import torch

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from neural_network_compression_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"nnc_cbwp_pack_bytes", "nnc_cbwp_pack", "nnc_cbwp_unpack", "nnc_cbwp_plan", "nnc_cbwp_workspace_bytes", "nnc_cbwp"}
STREAM, TILED, MFMA = nat.CBMM_STREAM, nat.CBMM_TILED, nat.CBMM_MFMA


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_symbols_header_and_signatures_agree(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nnc_cbwp.h")).read(), flags=re.S)
    protos = re.findall(r"\b(int64_t|int)\s+(nnc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    assert {p[1] for p in protos} == set(nat.WIDE_PACKED_SIGNATURES) == NAMES and len(protos) == len(NAMES)
    assert not set(nat.WIDE_PACKED_SIGNATURES) & set(nat.SIGNATURES)
    raw = ctypes.CDLL(nat.lib_path())
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "int32_t": ctypes.c_int32}
    for ret, name, args in protos:
        res, argtypes = nat.WIDE_PACKED_SIGNATURES[name]
        assert hasattr(raw, name) and res is ctype[ret]
        decl = [a.strip() for a in args.split(",")]
        assert len(decl) == len(argtypes), name
        for d, a in zip(decl, argtypes):
            assert (a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64))) if "*" in d else (a is ctype[d.split()[0]]), (name, d)
    assert os.path.join(nbuild.CSRC, "nnc_cbwp.hip") in nbuild.SOURCES
    assert len(nat.CBWP_PLAN_FIELDS) == int(re.search(r"#define NNC_CBWP_PLAN_LEN (\d+)", text).group(1))


@pytest.mark.parametrize("bits", [5, 6, 9])
@pytest.mark.parametrize("ncols", [1, 127, 128, 129, 300, 4096])
def test_pack_bytes_is_the_row_formula(lib, ncols, bits):
    base = 8 if bits == 9 else 4
    row = 16 * -(-ncols * base // 128) + (bits - base) * 16 * -(-ncols // 128)
    assert lib.nnc_cbwp_pack_bytes(1, ncols, bits) == row and lib.nnc_cbwp_pack_bytes(33, ncols, bits) == 33 * row
    assert ops.wide_packed_nbytes(33, ncols, bits) == 33 * row
    if ncols == 4096:
        assert row == {5: 2560, 6: 3072, 9: 4608}[bits]
    if (ncols, bits) == (300, 5):
        assert row == 208


def test_the_width_is_the_smallest_that_holds_k(lib):
    assert [ops.wide_packed_bits(k) for k in (17, 32, 33, 64, 65, 512)] == [5, 5, 6, 6, 9, 9]
    for k in (16, 513):
        with pytest.raises(ValueError):
            ops.wide_packed_bits(k)
    assert lib.nnc_cbwp_pack_bytes(4, 4, 4) == lib.nnc_cbwp_pack_bytes(4, 4, 8) == lib.nnc_cbwp_pack_bytes(-1, 4, 5) == 0


@pytest.mark.parametrize("cus", [80, 256, 304])
@pytest.mark.parametrize("bits,k", [(5, 17), (6, 64), (9, 257)])
def test_plan_invariants(lib, bits, k, cus):
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        for m in (1, 2, 3, 5, 9, 16, 17, 130, 4096):
            for kdim, ncols in ((1, 1), (33, 129), (200, 300), (2048, 127), (784, 300), (4096, 4096), (5000, 5000), (64, 100000)):
                p = ops.cbwp_plan(dtype, m, kdim, ncols, bits, k, cus)
                assert p["path"] == (STREAM if m <= 16 else TILED if dtype is torch.float32 else MFMA)
                assert 0 < p["lds"] <= 64 * 1024 and p["entries"] == 1 << bits and p["base"] + p["planes"] == bits
                assert p["splits"] >= 1 and p["rps"] * (p["splits"] - 1) < kdim <= p["rps"] * p["splits"]
                assert p["workspace"] == lib.nnc_cbwp_workspace_bytes(p["dtype"], m, kdim, ncols, bits) or cus != 256
                if m <= 16:
                    assert p["cols"] in (4, 8, 16, 32) and p["cols"] * p["base"] == 8 * p["vb"] and p["cols"] * p["mt"] <= 64 and p["mt"] >= m
                    assert p["col_tiles"] * 64 * p["cols"] >= ncols and p["copies"] * p["entries"] * 4 <= 32 * 1024


def test_argument_errors_come_back_without_a_device(lib):
    out = (ctypes.c_int64 * len(nat.CBWP_PLAN_FIELDS))()
    for args, msg in (((0, 4, 8, 16, 4, 16, 256, out), "bits must be 5, 6 or 9"), ((0, 4, 8, 16, 5, 33, 256, out), "k outside 1..2^bits"),
                      ((3, 4, 8, 16, 5, 17, 256, out), "x_dtype"), ((0, 4, 8, 16, 5, 17, 0, out), "cus < 1"), ((0, -1, 8, 16, 5, 17, 256, out), "negative size")):
        assert lib.nnc_cbwp_plan(*args) == -1 and msg in lib.nnc_last_error().decode()
    P = 0x1000
    nb = lib.nnc_cbwp_pack_bytes(8, 16, 5)
    assert lib.nnc_cbwp(P, 0, 4, 8, P, nb - 1, 5, 16, P, 17, None, 0, P, 0, None, 0, None) == -1 and "packed_bytes" in lib.nnc_last_error().decode()
    assert lib.nnc_cbwp(P, 0, 4, 8, P + 8, nb, 5, 16, P, 17, None, 0, P, 0, None, 0, None) == -1 and "16-byte aligned" in lib.nnc_last_error().decode()
    assert lib.nnc_cbwp(P, 0, 4, 8, P, nb, 5, 16, P, 17, None, 0, P, 1, None, 0, None) == -1 and "y_dtype" in lib.nnc_last_error().decode()
    assert lib.nnc_cbwp_unpack(P, lib.nnc_cbwp_pack_bytes(8, 16, 9), 9, 8, 16, P, 1, None) == -1 and "label_bytes_out = 2" in lib.nnc_last_error().decode()
    with pytest.raises(TypeError, match="CUDA"):
        ops.wide_packed_codebook_matmul(torch.zeros(3, 16), None, torch.zeros(17))
