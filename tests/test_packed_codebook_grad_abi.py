"""CPU checks of the packed codebook backward pass's C ABI (include/nnc.h, nnc_cbpk_dx_* / nnc_cbpk_dc_*): the symbols, the
argument errors (returned before any HIP call, so none of this needs a device; fake pointers, never dereferenced), the plans over
CU counts and shapes, the dc plan's agreement with the byte form's (the condition for bit-identical centroid gradients), that every
stream plan names a kernel that exists, that the case list of the GPU suite reaches every regime at several CU counts, the int64
bound of the fixed-point sums, and the argument checks of compress_network_trainable."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from neural_network_compression_amd import compressed, ops
from tests.helpers import packed_grad_ref as ref
from tests.helpers.packed_ref import PLAN_CUS

NNC_EINVAL, NNC_ENOSPACE = -1, -2
PATH_NONE, PATH_STREAM, PATH_TILED, PATH_ZERO = 0, 1, 2, 4
P = 0x10000          # a fake, 256-byte aligned address
SYMBOLS = ("nnc_cbpk_dx_workspace_bytes", "nnc_cbpk_dx_plan", "nnc_cbpk_dx_f32",
           "nnc_cbpk_dc_workspace_bytes", "nnc_cbpk_dc_plan", "nnc_cbpk_dc_f32")
# every k_cbpkdx_stream / k_cbpkdc_stream instantiation (csrc/nnc_cbpkgrad.hip, kPgCases) as (bits, vb, mt)
STREAM_INSTANCES = {(4, 16, 1), (4, 8, 1), (4, 4, 1), (4, 16, 2), (4, 8, 2), (4, 4, 2), (4, 8, 4), (4, 4, 4), (4, 4, 8), (4, 2, 16),
                    (2, 16, 1), (2, 8, 1), (2, 4, 1), (2, 8, 2), (2, 4, 2), (2, 4, 4), (2, 2, 8), (2, 1, 16)}


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_symbols_are_exported_and_bound(lib):
    raw = ctypes.CDLL(nat.lib_path())
    for s in SYMBOLS:
        assert hasattr(raw, s) and s in nat.SIGNATURES, s
    for name in ("packed_codebook_matmul_dx", "packed_codebook_centroid_grad", "packed_codebook_linear", "cbpk_dx_plan", "cbpk_dc_plan"):
        assert hasattr(ops, name), name
    for name in ("TrainablePackedCompressedDense", "TrainablePackedCompressedConv2D"):
        assert hasattr(compressed, name), name


def test_plan_constants_match_the_header(lib):
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nnc.h")).read()
    for prefix, n, fields in (("NNC_CBPKDX", nat.CBPKDX_PLAN_LEN, nat.CBPKDX_PLAN_FIELDS), ("NNC_CBPKDC", nat.CBPKDC_PLAN_LEN, nat.CBPKDC_PLAN_FIELDS)):
        defs = {k: int(v) for k, v in re.findall(r"#define (" + prefix + r"_\w+) (\d+)", text)}
        assert defs[prefix + "_PLAN_LEN"] == n == len(fields)
        for i, f in enumerate(fields):
            assert defs[prefix + "_P_" + f.upper()] == i, f


def _pack_bytes(lib, kdim, ncols, bits):
    return lib.nnc_cbpk_pack_bytes(max(kdim, 0), max(ncols, 0), bits if bits in (2, 4) else 4)


def dx_call(lib, g=P, m=4, kdim=8, packed=P, packed_bytes=None, bits=4, ncols=16, centers=P, k=16, dx=P, ws=P, ws_bytes=None):
    if packed_bytes is None:
        packed_bytes = _pack_bytes(lib, kdim, ncols, bits)
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbpk_dx_workspace_bytes(m, kdim, ncols, bits)
    return lib.nnc_cbpk_dx_f32(g, m, kdim, packed, packed_bytes, bits, ncols, centers, k, dx, ws, ws_bytes, None)


def dc_call(lib, x=P, g=P, m=4, kdim=8, packed=P, packed_bytes=None, bits=4, ncols=16, k=16, dc=P, f64=1, ws=P, ws_bytes=None):
    if packed_bytes is None:
        packed_bytes = _pack_bytes(lib, kdim, ncols, bits)
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbpk_dc_workspace_bytes(m, kdim, ncols, bits, k)
    return lib.nnc_cbpk_dc_f32(x, g, m, kdim, packed, packed_bytes, bits, ncols, k, dc, f64, ws, ws_bytes, None)


BAD = [dict(m=-1), dict(kdim=-1), dict(ncols=-1), dict(k=0), dict(k=17), dict(k=5, bits=2), dict(bits=0), dict(bits=1), dict(bits=3),
       dict(bits=8), dict(m=(1 << 40) + 1), dict(packed=None), dict(packed=P + 8), dict(packed=P + 4), dict(packed_bytes=100),
       dict(packed_bytes=8 * 16 + 16), dict(ws_bytes=-1), dict(kdim=1 << 41), dict(ncols=(1 << 40) + 1)]


@pytest.mark.parametrize("kw", BAD + [dict(centers=None), dict(dx=None), dict(g=None), dict(m=16, kdim=64, ncols=5000, ws=None),
                                      dict(m=16, kdim=64, ncols=5000, ws=P + 2)])
def test_dx_bad_arguments_are_einval_without_a_device(lib, kw):
    assert dx_call(lib, **kw) == NNC_EINVAL
    assert lib.nnc_last_error()


@pytest.mark.parametrize("kw", BAD + [dict(x=None), dict(g=None), dict(dc=None), dict(ws=None), dict(ws=P + 4)])
def test_dc_bad_arguments_are_einval_without_a_device(lib, kw):
    assert dc_call(lib, **kw) == NNC_EINVAL
    assert lib.nnc_last_error()


def test_short_workspace_is_enospace_without_a_device(lib):
    for bits in (2, 4):
        for m in (1, 16, 300):
            need = lib.nnc_cbpk_dx_workspace_bytes(m, 5000, 5000, bits)
            assert need >= 2 * m * 5000 * 4                    # several column blocks (m <= 16) or splits of ncols
            assert dx_call(lib, m=m, kdim=5000, ncols=5000, bits=bits, k=4, ws_bytes=need - 1) == NNC_ENOSPACE
        need = lib.nnc_cbpk_dc_workspace_bytes(1, 5000, 5000, bits, 4)
        assert need == 64 + 8 * 4
        assert dc_call(lib, m=1, kdim=5000, ncols=5000, bits=bits, k=4, ws_bytes=need - 1) == NNC_ENOSPACE


@pytest.mark.parametrize("plan", [ops.cbpk_dx_plan, ops.cbpk_dc_plan])
def test_plan_argument_errors(lib, plan):
    for args in ((4, 8, 16, 4, 16, 0), (4, 8, 16, 4, 17, 64), (4, 8, 16, 2, 5, 64), (4, 8, 16, 0, 16, 64), (4, 8, 16, 3, 4, 64),
                 (4, 1 << 41, 16, 4, 16, 64), (-1, 8, 16, 4, 16, 64), (4, 8, 16, 4, 0, 64)):
        with pytest.raises(nat.NncError):
            plan(*args)
    assert lib.nnc_cbpk_dx_plan(4, 8, 16, 4, 16, 64, None) == NNC_EINVAL
    assert lib.nnc_cbpk_dc_plan(4, 8, 16, 4, 16, 64, None) == NNC_EINVAL
    assert lib.nnc_cbpk_dx_workspace_bytes(4, 1 << 41, 16, 4) == 0 and lib.nnc_cbpk_dc_workspace_bytes(4, 8, 16, 3, 4) == 0


MS = (0, 1, 2, 3, 7, 8, 15, 16, 17, 127, 128, 255, 256, 300, 4096)      # both sides of m = 16 and of every split of m (16 TB_K = 128)
DIMS = (0, 1, 63, 65, 127, 128, 129, 255, 256, 1000, 5000, 8192)         # ... and of the splits of ncols


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("bits,k", [(2, 1), (2, 4), (4, 5), (4, 16)])
def test_plans_are_consistent_over_cu_counts_and_take_splits_and_terms_from_the_byte_dc_plan(lib, m, bits, k):
    for kdim in DIMS:
        for ncols in DIMS:
            dx0 = dc0 = None
            for cus in PLAN_CUS:
                dx = ops.cbpk_dx_plan(m, kdim, ncols, bits, k, cus)
                dc = ops.cbpk_dc_plan(m, kdim, ncols, bits, k, cus)
                # everything but the number of row groups depends on the shape alone
                key_dx = tuple(v for f, v in dx.items() if f != "row_tiles")
                key_dc = tuple(v for f, v in dc.items() if f != "row_tiles")
                dx0, dc0 = dx0 or key_dx, dc0 or key_dc
                assert key_dx == dx0 and key_dc == dc0, (m, kdim, ncols, cus)
                assert dx["workspace"] == lib.nnc_cbpk_dx_workspace_bytes(m, kdim, ncols, bits)
                assert dc["workspace"] == lib.nnc_cbpk_dc_workspace_bytes(m, kdim, ncols, bits, k)
                assert dx["lds"] <= 64 * 1024 and dc["lds"] <= 64 * 1024
                if m == 0 or kdim == 0:
                    assert dx["path"] == PATH_NONE and dx["workspace"] == 0
                elif ncols == 0:
                    assert dx["path"] == PATH_ZERO and dx["workspace"] == 0
                if m * kdim * ncols == 0:
                    assert dc["path"] == PATH_ZERO and dc["workspace"] == 0
                    continue
                # S is the byte form's: the same splits of m, the same T
                byte = ops.cbmm_dc_plan(m, kdim, ncols, 1, k, cus)
                assert (dc["splits"], dc["rps"], dc["terms_log2"]) == (byte["splits"], byte["rps"], byte["terms_log2"])
                assert dc["workspace"] == byte["workspace"] == 64 + 8 * k
                assert dx["workspace"] == (dx["splits"] * m * kdim * 4 if dx["splits"] > 1 else 0)
                assert dc["copies"] == 64 and dx["entries"] == 1 << bits
                if m <= 16:
                    assert dx["path"] == dc["path"] == PATH_STREAM
                    for p in (dx, dc):
                        assert (bits, p["vb"], p["mt"]) in STREAM_INSTANCES
                        assert p["mt"] >= m and p["cols"] == 8 * p["vb"] // bits and p["cols"] * p["mt"] <= 64
                        assert p["col_tiles"] * 64 * p["cols"] >= ncols > (p["col_tiles"] - 1) * 64 * p["cols"]
                        assert 1 <= p["row_tiles"] <= max(1, 2 * min(cus, 256)) and p["row_tiles"] <= kdim
                    assert (dx["vb"], dx["mt"], dx["col_tiles"], dx["row_tiles"]) == (dc["vb"], dc["mt"], dc["col_tiles"], dc["row_tiles"])
                    assert dx["splits"] == dx["col_tiles"] and dx["cps"] == 64 * dx["cols"] and dc["splits"] == 1
                    assert dx["copies"] == 32 and dx["lds"] == (32 * dx["entries"] + dx["entries"]) * 4
                    assert dc["lds"] == k * 64 * 8
                else:
                    assert dx["path"] == dc["path"] == PATH_TILED
                    assert dx["col_tiles"] * 128 >= kdim and dx["row_tiles"] * 128 >= m
                    assert dc["col_tiles"] * 128 >= ncols and dc["row_tiles"] * 128 >= kdim
                    assert dx["cps"] % 16 == 0 and 1 <= dx["splits"] <= 16
                    assert dx["splits"] * dx["cps"] >= ncols > (dx["splits"] - 1) * dx["cps"]
                    assert dc["splits"] * dc["rps"] >= m > (dc["splits"] - 1) * dc["rps"]


@pytest.mark.parametrize("bits", [2, 4])
def test_every_stream_plan_names_an_instantiation_that_exists(lib, bits):
    """m = 1..16, ncols from 1 to beyond two column blocks of the widest load: a plan without a kernel would be NNC_EINVAL here."""
    seen = set()
    ncols_list = sorted(set(list(range(1, 140)) + [n + d for n in (256, 512, 1024, 2048, 4096, 8192, 3 * 4096) for d in (-1, 0, 1)]
                            + [300, 5000, 2 * 64 * 128 // bits + 1]))
    for m in range(1, 17):
        for ncols in ncols_list:
            for kdim in (1, 700, 20000):                     # (the widest loads need kdim / 32 row groups to fill the planning device)
                dx = ops.cbpk_dx_plan(m, kdim, ncols, bits, 1 << bits, 256)
                dc = ops.cbpk_dc_plan(m, kdim, ncols, bits, 1 << bits, 256)
                assert (bits, dx["vb"], dx["mt"]) in STREAM_INSTANCES and (dx["vb"], dx["mt"]) == (dc["vb"], dc["mt"]), (m, ncols)
                seen.add((bits, dx["vb"], dx["mt"]))
    assert seen == {c for c in STREAM_INSTANCES if c[0] == bits}      # and no instantiation is an orphan


@pytest.mark.parametrize("cus", PLAN_CUS)
def test_the_case_list_covers_every_regime(lib, cus):
    ref.assert_covered(ops, cus)
    for case in ref.CASES:
        name, m, kdim, ncols, bits, k = case
        dxp, dcp = ops.cbpk_dx_plan(m, kdim, ncols, bits, k, cus), ops.cbpk_dc_plan(m, kdim, ncols, bits, k, cus)
        if name.startswith("stream"):       # the case hits the regime its name claims
            assert dxp["path"] == dcp["path"] == PATH_STREAM
            assert ("oneblock" not in name) or dxp["splits"] == 1
            assert ("blocks" not in name) or dxp["splits"] > 1
        elif name.startswith("tiled"):
            assert dxp["path"] == dcp["path"] == PATH_TILED
            assert ("nosplit" not in name) or dxp["splits"] == 1
            assert ("_split" not in name) or dxp["splits"] > 1
            assert ("msplit" in name) == (dcp["splits"] > 1)


@pytest.mark.parametrize("m,kdim,ncols", [(1, 1, 1), (16, 5000, 5000), (1 << 40, 1, 1), (4096, 1 << 20, 1 << 20), (300, 8192, 8192),
                                          (17, 1 << 34, 64), (16, 1 << 40, 16)])
@pytest.mark.parametrize("ax,ag", [(1.0, 1.0), (3.4e38, 1e-30), (1e-30, 1e-30), (2.0 ** 60, 2.0 ** -3), (65504.0, 65504.0)])
def test_the_bound_keeps_the_integer_sums_in_int64(lib, m, kdim, ncols, ax, ag):
    """Every image rint(dW 2^S) is at most 2^(P+S) (1 + u)^m and there are at most 2^T of them in all: a lane's copy of an LDS
    bin, a workgroup's bins and the global sums each hold a subset of them, so |sum| < 2^62 (1 + u)^m, in exact rational
    arithmetic.  (There are no per-lane register bins.)"""
    for bits, k in ((2, 4), (4, 16)):
        plan = ops.cbpk_dc_plan(m, kdim, ncols, bits, k, 256)
        t = plan["terms_log2"]
        assert (1 << t) >= kdim * ncols * plan["splits"]
        S, flag = ops.cbgrad_shift(m, ax, ag, t)
        if flag != ops.CBGRAD_OK:
            continue
        bound = Fraction(float(m) * float(np.float32(ax)) * float(np.float32(ag)))
        P_ = 62 - t - S
        assert Fraction(2) ** P_ > bound
        assert (kdim * ncols * plan["splits"]) * Fraction(2) ** (P_ + S) <= Fraction(2) ** 62


@pytest.mark.parametrize("m,kdim,ncols,dxp,dcp", [(0, 5, 5, PATH_NONE, PATH_ZERO), (3, 0, 5, PATH_NONE, PATH_ZERO),
                                                  (3, 5, 0, PATH_ZERO, PATH_ZERO), (30, 5, 0, PATH_ZERO, PATH_ZERO)])
def test_empty_shapes_plan(lib, m, kdim, ncols, dxp, dcp):
    for bits in (2, 4):
        assert ops.cbpk_dx_plan(m, kdim, ncols, bits, 4, 256)["path"] == dxp
        assert ops.cbpk_dc_plan(m, kdim, ncols, bits, 4, 256)["path"] == dcp
        assert lib.nnc_cbpk_dx_workspace_bytes(m, kdim, ncols, bits) == 0 and lib.nnc_cbpk_dc_workspace_bytes(m, kdim, ncols, bits, 4) == 0


def test_compress_network_trainable_checks_packed_before_it_touches_the_network(lib):
    for bad in (None, "yes", "byte", 2.0):
        with pytest.raises(ValueError, match="packed"):
            compressed.compress_network_trainable(None, {}, packed=bad)
    with pytest.raises(ValueError, match="sparse=True and packed=True"):
        compressed.compress_network_trainable(None, {}, sparse=True, packed=True)
    with pytest.raises(ValueError, match="inference only.*compress_network_trainable"):
        compressed.compress_network(None, {}, trainable=True, packed=True)
    with pytest.raises(ValueError, match="inference only"):
        compressed.compress_network(None, {}, trainable=True, packed="auto")


def test_packed_codebook_linear_rejects_codes_that_are_not_packed(lib):
    with pytest.raises(TypeError, match="PackedCodes"):
        ops.packed_codebook_linear(None, object(), None)
