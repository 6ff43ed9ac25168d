"""CPU checks of the bitmap-sparse codebook backward pass's C ABI (include/nnc.h, nnc_cbsp_dx_* / nnc_cbsp_dc_*): the symbols, the
argument errors (returned before any HIP call, so none of this needs a device; fake pointers, never dereferenced), the plans over
CU counts and shapes, the dc plan's agreement with the dense one (the condition for bit-identical centroid gradients), the int64
bound of the fixed-point sums, and the argument check of compress_network_trainable."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from neural_network_compression_amd import compressed, ops

NNC_EINVAL, NNC_ENOSPACE = -1, -2
PATH_NONE, PATH_STREAM, PATH_TILED, PATH_ZERO = 0, 1, 2, 4
P = 0x10000          # a fake, 256-byte aligned address
SYMBOLS = ("nnc_cbsp_dx_workspace_bytes", "nnc_cbsp_dx_plan", "nnc_cbsp_dx_f32",
           "nnc_cbsp_dc_workspace_bytes", "nnc_cbsp_dc_plan", "nnc_cbsp_dc_f32")


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_symbols_are_exported_and_bound(lib):
    raw = ctypes.CDLL(nat.lib_path())
    for s in SYMBOLS:
        assert hasattr(raw, s) and s in nat.SIGNATURES, s
    for name in ("sparse_codebook_matmul_dx", "sparse_codebook_centroid_grad", "sparse_codebook_linear", "cbsp_dx_plan", "cbsp_dc_plan"):
        assert hasattr(ops, name), name
    for name in ("TrainableSparseCompressedDense", "TrainableSparseCompressedConv2D", "compress_network_trainable"):
        assert hasattr(compressed, name), name


def test_plan_constants_match_the_header():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nnc.h")).read()
    for prefix, n, fields in (("NNC_CBSPDX", nat.CBSPDX_PLAN_LEN, nat.CBSPDX_PLAN_FIELDS), ("NNC_CBSPDC", nat.CBSPDC_PLAN_LEN, nat.CBSPDC_PLAN_FIELDS)):
        defs = {k: int(v) for k, v in re.findall(r"#define (" + prefix + r"_\w+) (\d+)", text)}
        assert defs[prefix + "_PLAN_LEN"] == n == len(fields)
        for i, f in enumerate(fields):
            assert defs[prefix + "_P_" + f.upper()] == i, f


def dx_call(lib, g=P, m=4, kdim=8, packed=P, packed_bytes=None, lb=1, ncols=16, z=0, nnz=0, centers=P, k=16, dx=P, ws=P, ws_bytes=None):
    if packed_bytes is None:
        packed_bytes = lib.nnc_cbsp_pack_bytes(max(kdim, 0), max(ncols, 0), lb if lb in (1, 2) else 1, max(nnz, 0))
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbsp_dx_workspace_bytes(m, kdim, ncols, lb)
    return lib.nnc_cbsp_dx_f32(g, m, kdim, packed, packed_bytes, lb, ncols, z, nnz, centers, k, dx, ws, ws_bytes, None)


def dc_call(lib, x=P, g=P, m=4, kdim=8, packed=P, packed_bytes=None, lb=1, ncols=16, z=0, nnz=0, k=16, dc=P, f64=1, ws=P, ws_bytes=None):
    if packed_bytes is None:
        packed_bytes = lib.nnc_cbsp_pack_bytes(max(kdim, 0), max(ncols, 0), lb if lb in (1, 2) else 1, max(nnz, 0))
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbsp_dc_workspace_bytes(m, kdim, ncols, lb, k) if 1 <= k <= 1040 else 0
    return lib.nnc_cbsp_dc_f32(x, g, m, kdim, packed, packed_bytes, lb, ncols, z, nnz, k, dc, f64, ws, ws_bytes, None)


BAD = [dict(m=-1), dict(kdim=-1), dict(ncols=-1), dict(k=0), dict(k=1041, lb=2), dict(lb=0), dict(lb=3), dict(k=257, lb=1),
       dict(m=1 << 41), dict(z=-1), dict(z=256), dict(z=65536, lb=2), dict(nnz=-1), dict(nnz=8 * 16 + 1), dict(packed=None),
       dict(packed=P + 16), dict(packed_bytes=100), dict(ws_bytes=-1), dict(kdim=1 << 35, ncols=4096)]


@pytest.mark.parametrize("kw", BAD + [dict(centers=None), dict(dx=None), dict(g=None), dict(ws=None), dict(ws=P + 2)])
def test_dx_bad_arguments_are_einval_without_a_device(lib, kw):
    assert dx_call(lib, **kw) == NNC_EINVAL
    assert lib.nnc_last_error()


@pytest.mark.parametrize("kw", BAD + [dict(x=None), dict(g=None), dict(dc=None), dict(ws=None), dict(ws=P + 4)])
def test_dc_bad_arguments_are_einval_without_a_device(lib, kw):
    assert dc_call(lib, **kw) == NNC_EINVAL
    assert lib.nnc_last_error()


def test_short_workspace_is_enospace_without_a_device(lib):
    for m in (1, 16, 300):
        need = lib.nnc_cbsp_dx_workspace_bytes(m, 5000, 5000, 1)
        assert need >= m * 4
        assert dx_call(lib, m=m, kdim=5000, ncols=5000, ws_bytes=need - 1) == NNC_ENOSPACE
    need = lib.nnc_cbsp_dc_workspace_bytes(1, 5000, 5000, 2, 1040)
    assert need == 64 + 8 * 1040
    assert dc_call(lib, m=1, kdim=5000, ncols=5000, lb=2, k=1040, ws_bytes=need - 1) == NNC_ENOSPACE


@pytest.mark.parametrize("plan", [ops.cbsp_dx_plan, ops.cbsp_dc_plan])
def test_plan_argument_errors(lib, plan):
    for args in ((4, 8, 16, 1, 16, 0), (4, 8, 16, 1, 300, 64), (4, 8, 16, 0, 16, 64), (4, 8, 16, 3, 16, 64), (4, 1 << 35, 4096, 1, 16, 64),
                 (-1, 8, 16, 1, 16, 64)):
        with pytest.raises(nat.NncError):
            plan(*args)
    assert lib.nnc_cbsp_dx_plan(4, 8, 16, 1, 16, 64, None) == NNC_EINVAL
    assert lib.nnc_cbsp_dc_plan(4, 8, 16, 1, 16, 64, None) == NNC_EINVAL
    assert lib.nnc_cbsp_dx_workspace_bytes(4, 1 << 35, 4096, 1) == 0 and lib.nnc_cbsp_dc_workspace_bytes(4, 8, 16, 3, 16) == 0


MS = (0, 1, 7, 16, 17, 300, 4096)
DIMS = (0, 1, 63, 65, 129, 1000, 5000, 8192)
CUS = (1, 80, 256, 304)


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("lb,k", [(1, 1), (1, 256), (2, 257), (2, 1040)])
def test_plans_are_consistent_over_cu_counts_and_match_the_dense_dc_plan(lib, m, lb, k):
    for kdim in DIMS:
        for ncols in DIMS:
            dx0 = dc0 = None
            for cus in CUS:
                dx = ops.cbsp_dx_plan(m, kdim, ncols, lb, k, cus)
                dc = ops.cbsp_dc_plan(m, kdim, ncols, lb, k, cus)
                # the splits (so the bits) and the workspace depend on the shape alone
                key_dx = (dx["path"], dx["splits"], dx["cps"], dx["mt"], dx["segs"], dx["workspace"])
                key_dc = (dc["path"], dc["splits"], dc["rps"], dc["terms_log2"], dc["copies"], dc["workspace"])
                dx0, dc0 = dx0 or key_dx, dc0 or key_dc
                assert key_dx == dx0 and key_dc == dc0, (m, kdim, ncols, cus)
                assert dx["workspace"] == lib.nnc_cbsp_dx_workspace_bytes(m, kdim, ncols, lb)
                assert dc["workspace"] == lib.nnc_cbsp_dc_workspace_bytes(m, kdim, ncols, lb, k)
                assert dx["lds"] <= 64 * 1024 and dc["lds"] <= 64 * 1024
                if m == 0 or kdim == 0:
                    assert dx["path"] == PATH_NONE and dx["workspace"] == 0
                elif ncols == 0:
                    assert dx["path"] == PATH_ZERO and dx["workspace"] == 0
                if m * kdim * ncols == 0:
                    assert dc["path"] == PATH_ZERO and dc["workspace"] == 0
                    continue
                # the dc plan is the dense one's where it matters: the same S, so the same images
                dense = ops.cbmm_dc_plan(m, kdim, ncols, lb, k, cus)
                assert (dc["splits"], dc["rps"], dc["terms_log2"], dc["copies"]) == \
                       (dense["splits"], dense["rps"], dense["terms_log2"], dense["copies"])
                assert dc["workspace"] == dense["workspace"] == 64 + 8 * k
                segs = -(-ncols // 64)
                part = dx["splits"] * m * kdim * 4 if dx["splits"] > 1 else 0
                assert dx["workspace"] == (part + 255) // 256 * 256 + m * 4
                if m <= 16:
                    assert dx["path"] == dc["path"] == PATH_STREAM
                    assert dx["mt"] >= m and dx["mt"] * dx["segs"] <= max(32, dx["mt"] * 8) and 64 % dx["segs"] == 0
                    assert dx["col_tiles"] * dx["segs"] >= segs > (dx["col_tiles"] - 1) * dx["segs"]
                    assert dx["splits"] == dx["col_tiles"] and dx["cps"] == 64 * dx["segs"] and dc["splits"] == 1
                    assert 1 <= dx["row_tiles"] <= max(1, 2 * min(cus, 256)) and dx["row_tiles"] <= kdim
                    assert dx["entries"] == (256 if lb == 1 else k + 1)
                    assert dx["copies"] * dx["entries"] * 4 + dx["entries"] * 4 == dx["lds"]
                else:
                    assert dx["path"] == dc["path"] == PATH_TILED
                    assert dx["col_tiles"] * 128 >= kdim and dx["row_tiles"] * 128 >= m
                    assert dc["col_tiles"] * 128 >= ncols and dc["row_tiles"] * 128 >= kdim
                    assert dx["cps"] % 64 == 0 and 1 <= dx["splits"] <= 16
                    assert dx["splits"] * dx["cps"] >= ncols > (dx["splits"] - 1) * dx["cps"]


@pytest.mark.parametrize("m,kdim,ncols", [(1, 1, 1), (16, 5000, 5000), (1 << 40, 1, 1), (4096, 1 << 20, 1 << 20), (300, 8192, 8192),
                                          (17, 1 << 34, 64)])
@pytest.mark.parametrize("ax,ag", [(1.0, 1.0), (3.4e38, 1e-30), (1e-30, 1e-30), (2.0 ** 60, 2.0 ** -3), (65504.0, 65504.0)])
def test_the_bound_keeps_the_integer_sums_in_int64(m, kdim, ncols, ax, ag):
    """Every image rint(dW 2^S) is at most 2^(P+S) (1 + u)^m and there are at most 2^T of them (skipped positions included:
    the per-lane register for bin z holds a subset of them): |sum| < 2^62 (1 + u)^m, in exact rational arithmetic."""
    lb, k = 2, 1040
    plan = ops.cbsp_dc_plan(m, kdim, ncols, lb, k, 256)
    t = plan["terms_log2"]
    assert (1 << t) >= kdim * ncols * plan["splits"]
    S, flag = ops.cbgrad_shift(m, ax, ag, t)
    if flag != ops.CBGRAD_OK:
        return
    bound = Fraction(float(m) * float(np.float32(ax)) * float(np.float32(ag)))
    P_ = 62 - t - S
    assert Fraction(2) ** P_ > bound
    assert (kdim * ncols * plan["splits"]) * Fraction(2) ** (P_ + S) <= Fraction(2) ** 62


@pytest.mark.parametrize("m,kdim,ncols,dxp,dcp", [(0, 5, 5, PATH_NONE, PATH_ZERO), (3, 0, 5, PATH_NONE, PATH_ZERO),
                                                  (3, 5, 0, PATH_ZERO, PATH_ZERO), (30, 5, 0, PATH_ZERO, PATH_ZERO)])
def test_empty_shapes_plan(lib, m, kdim, ncols, dxp, dcp):
    assert ops.cbsp_dx_plan(m, kdim, ncols, 1, 4, 256)["path"] == dxp
    assert ops.cbsp_dc_plan(m, kdim, ncols, 1, 4, 256)["path"] == dcp
    assert lib.nnc_cbsp_dx_workspace_bytes(m, kdim, ncols, 1) == 0 and lib.nnc_cbsp_dc_workspace_bytes(m, kdim, ncols, 1, 4) == 0


@pytest.mark.parametrize("bad", [None, "yes", "dense", 2.0])
def test_compress_network_trainable_rejects_a_bad_sparse_value(bad):
    with pytest.raises(ValueError, match="sparse"):
        compressed.compress_network_trainable(None, {}, sparse=bad)
