"""CPU checks of the C ABI of the backward pass of the 5-, 6- and 9-bit split-plane ("wide packed") codebook layer
(include/nnc_cbwpgrad.h): the header against the bound signatures, the argument errors and the invariants of
the two plans.  No device needed."""
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
WIDTHS = [(5, 17), (6, 64), (9, 257)]


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_symbols_header_and_signatures_agree(lib):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nnc_cbwpgrad.h")).read(), flags=re.S)
    protos = re.findall(r"\b(int64_t|int)\s+(nnc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    assert {p[1] for p in protos} == set(nat.WIDE_PACKED_GRAD_SIGNATURES) and len(protos) == 6
    assert not set(nat.WIDE_PACKED_GRAD_SIGNATURES) & (set(nat.SIGNATURES) | set(nat.WIDE_PACKED_SIGNATURES) | set(nat.PACKED_H16_SIGNATURES))
    raw = ctypes.CDLL(nat.lib_path())
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "int32_t": ctypes.c_int32}
    for ret, name, args in protos:
        res, argtypes = nat.WIDE_PACKED_GRAD_SIGNATURES[name]
        assert hasattr(raw, name) and res is ctype[ret]
        decl = [a.strip() for a in args.split(",")]
        assert len(decl) == len(argtypes), name
        for d, a in zip(decl, argtypes):
            assert (a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64))) if "*" in d else (a is ctype[d.split()[0]]), (name, d)
    assert os.path.join(nbuild.CSRC, "nnc_cbwpgrad.hip") in nbuild.SOURCES
    for fields, macro in ((nat.CBWPDX_PLAN_FIELDS, "NNC_CBWPDX"), (nat.CBWPDC_PLAN_FIELDS, "NNC_CBWPDC")):
        assert len(fields) == int(re.search(rf"#define {macro}_PLAN_LEN (\d+)", text).group(1))
        assert [f.upper() for f in fields] == [n for n, _ in sorted(re.findall(rf"#define {macro}_P_(\w+) (\d+)", text), key=lambda t: int(t[1]))]


def test_argument_errors_come_back_without_a_device(lib):
    out = (ctypes.c_int64 * len(nat.CBWPDX_PLAN_FIELDS))()
    for plan in (lib.nnc_cbwp_dx_plan, lib.nnc_cbwp_dc_plan):
        for args, msg in (((0, 4, 8, 16, 4, 16, 256, out), "bits must be 5, 6 or 9"), ((0, 4, 8, 16, 5, 33, 256, out), "k outside 1..2^bits"),
                          ((3, 4, 8, 16, 5, 17, 256, out), "x_dtype"), ((0, 4, 8, 16, 5, 17, 0, out), "cus < 1"),
                          ((0, -1, 8, 16, 5, 17, 256, out), "negative size"), ((0, 4, 8, 16, 5, 17, 256, None), "out is NULL")):
            assert plan(*args) == -1 and msg in lib.nnc_last_error().decode()
    P, nb = 0x1000, lib.nnc_cbwp_pack_bytes(8, 16, 5)
    err = lambda: lib.nnc_last_error().decode()                                                   # noqa: E731
    assert lib.nnc_cbwp_dx(P, 0, 4, 8, P, nb - 1, 5, 16, P, 17, P, 0, None, 0, None) == -1 and "packed_bytes" in err()
    assert lib.nnc_cbwp_dx(P, 0, 4, 8, P + 8, nb, 5, 16, P, 17, P, 0, None, 0, None) == -1 and "16-byte aligned" in err()
    assert lib.nnc_cbwp_dx(P, 0, 4, 8, P, nb, 5, 16, P, 17, P, 1, None, 0, None) == -1 and "dx_dtype" in err()
    assert lib.nnc_cbwp_dx(P, 1, 4, 8, P, nb, 5, 16, P, 17, P, 2, None, 0, None) == -1 and "dx_dtype" in err()
    assert lib.nnc_cbwp_dx(P + 1, 1, 4, 8, P, nb, 5, 16, P, 17, P, 1, None, 0, None) == -1 and "not aligned" in err()
    assert lib.nnc_cbwp_dx(P, 0, 4, 8, P, nb, 5, 16, None, 17, P, 0, None, 0, None) == -1 and "centers is NULL" in err()
    assert lib.nnc_cbwp_dc(P, P + 1, 2, 4, 8, P, nb, 5, 16, 17, P, 1, P, 1 << 20, None) == -1 and "not aligned" in err()
    assert lib.nnc_cbwp_dc(P, P, 0, 4, 8, P, nb, 5, 16, 17, None, 1, P, 1 << 20, None) == -1 and "dc is NULL" in err()
    assert lib.nnc_cbwp_dc(P, P, 0, 4, 8, P, nb, 5, 16, 17, P, 1, P, 8, None) == -2 and "workspace" in err()          # NNC_ENOSPACE
    nb = lib.nnc_cbwp_pack_bytes(200, 1100, 5)
    assert lib.nnc_cbwp_dx(P, 0, 16, 200, P, nb, 5, 1100, P, 17, P, 0, P, 8, None) == -2 and "workspace" in err()
    for fn in (ops.wide_packed_codebook_matmul_dx, ops.wide_packed_codebook_linear):
        with pytest.raises(TypeError, match="CUDA|WidePackedCodes"):
            fn(torch.zeros(3, 16), None, torch.zeros(17))


@pytest.mark.parametrize("cus", [80, 256, 304])
@pytest.mark.parametrize("bits,k", WIDTHS)
def test_plan_invariants(lib, bits, k, cus):
    lb = 2 if bits == 9 else 1
    for dtype in DTYPES:
        tile = TILED if dtype is torch.float32 else MFMA
        for m in (1, 3, 16, 17, 130, 4096):
            for kdim, ncols in ((1, 1), (33, 129), (200, 300), (200, 1100), (2048, 127), (4096, 4096), (5000, 5000), (64, 100000)):
                dx, dc = ops.cbwp_dx_plan(dtype, m, kdim, ncols, bits, k, cus), ops.cbwp_dc_plan(dtype, m, kdim, ncols, bits, k, cus)
                byte = (ops.cbmm_dc_plan(m, kdim, ncols, lb, k, cus) if dtype is torch.float32
                        else ops.cbmm_dc_h16_plan(dtype, m, kdim, ncols, lb, k, cus))
                assert dx["path"] == dc["path"] == byte["path"] == (STREAM if m <= 16 else tile)
                assert (dc["splits"], dc["rps"], dc["terms_log2"]) == (byte["splits"], byte["rps"], byte["terms_log2"])
                assert dx["entries"] == 1 << bits and dc["copies"] == byte["copies"] == (32 if k <= 64 else 2)
                for p, extent, per in ((dx, ncols, "cps"), (dc, m, "rps")):
                    assert 0 < p["lds"] <= 64 * 1024 and p["base"] + p["planes"] == bits
                    assert p["splits"] >= 1 and p[per] * (p["splits"] - 1) < extent <= p[per] * p["splits"]
                    assert p["dtype"] == ops._X_DT[dtype]
                    if m <= 16:
                        assert p["cols"] in (4, 8, 16, 32) and p["cols"] * p["base"] == 8 * p["vb"] and p["cols"] * p["mt"] <= 64 and p["mt"] >= m
                        assert p["col_tiles"] * 64 * p["cols"] >= ncols
                    else:
                        assert p["vb"] == p["mt"] == p["cols"] == 0
                if m > 16:
                    assert dx["cps"] % 32 == 0
                if cus == 256:
                    assert dx["workspace"] == lib.nnc_cbwp_dx_workspace_bytes(dx["dtype"], m, kdim, ncols, bits)
                    assert dc["workspace"] == lib.nnc_cbwp_dc_workspace_bytes(dc["dtype"], m, kdim, ncols, bits, k) == 64 + 8 * k
                else:   # the splits depend on the shape alone
                    assert dx["splits"] == ops.cbwp_dx_plan(dtype, m, kdim, ncols, bits, k, 256)["splits"]


@pytest.mark.parametrize("bits,k", WIDTHS)
def test_the_empty_shapes_launch_nothing(lib, bits, k):
    for dtype in DTYPES:
        assert ops.cbwp_dx_plan(dtype, 0, 8, 16, bits, k, 256)["path"] == ops.cbwp_dx_plan(dtype, 4, 0, 16, bits, k, 256)["path"] == nat.CBMM_NONE
        assert ops.cbwp_dx_plan(dtype, 20, 8, 0, bits, k, 256)["path"] == nat.CBMM_ZERO
        assert {ops.cbwp_dc_plan(dtype, *s, bits, k, 256)["path"] for s in ((0, 8, 16), (4, 0, 16), (20, 8, 0))} == {nat.CBMM_ZERO}


@pytest.mark.parametrize("bits,k", WIDTHS)
def test_the_gpu_shapes_split_every_path(lib, bits, k):
    """The shapes of tests/test_gpu_zzzzzz_wide_packed_backward.py reach two or more splits on each kernel that has them; m = 300 is the
    added one: the float32 dc tile splits m only from 256 rows (m / 128 >= 2)."""
    f32, bf16 = torch.float32, torch.bfloat16
    p = ops.cbwp_dx_plan(f32, 16, 200, 1100, bits, k, 256)
    assert p["path"] == STREAM and p["splits"] >= 2
    p = ops.cbwp_dx_plan(f32, 130, 200, 300, bits, k, 256)
    assert p["path"] == TILED and p["splits"] >= 2
    p = ops.cbwp_dx_plan(bf16, 130, 200, 300, bits, k, 256)
    assert p["path"] == MFMA and p["splits"] >= 2
    assert ops.cbwp_dc_plan(f32, 130, 200, 300, bits, k, 256)["splits"] == 1
    p = ops.cbwp_dc_plan(f32, 300, 200, 300, bits, k, 256)
    assert p["path"] == TILED and p["splits"] >= 2
    p = ops.cbwp_dc_plan(bf16, 130, 200, 300, bits, k, 256)
    assert p["path"] == MFMA and p["splits"] >= 2
