"""CPU checks of the C ABI of the half-precision codebook backward pass (include/nnc_cbgrad_h16.h, nnc_cbmm_dx_h16 /
nnc_cbmm_dc_h16): the header against the bound signatures, the plans over CU counts, the regimes the case list
of tests/helpers/h16_grad_ref.py hits, the fixed-point bound at the extreme shapes, every argument error (returned before any HIP
call, so none of this needs a device) and the Python errors that need none."""
import ctypes
import os
import re
from fractions import Fraction

import pytest
import torch

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from neural_network_compression_amd import compressed, ops
from tests.helpers import h16_grad_ref as href
from tests.helpers import h16_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NNC_EINVAL, NNC_ENOSPACE = -1, -2
P = 0x1000   # a fake, never dereferenced address
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
CUS = (1, 2, 7, 64, 80, 255, 256, 257, 304, 1024)


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_symbols_header_and_signatures_agree(lib):
    """every prototype of include/nnc_cbgrad_h16.h is exported and bound with as many arguments as it declares; nnc.h includes it"""
    text = open(os.path.join(ROOT, "include", "nnc_cbgrad_h16.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(int64_t|int)\s+(nnc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    assert {p[1] for p in protos} == set(nat.H16_GRAD_SIGNATURES) and len(protos) == 6
    raw = ctypes.CDLL(nat.lib_path())
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64}
    for ret, name, args in protos:
        res, argtypes = nat.H16_GRAD_SIGNATURES[name]
        assert hasattr(raw, name) and res is ctype[ret]
        decl = [a.strip() for a in args.split(",")]
        assert len(decl) == len(argtypes), name
        for d, a in zip(decl, argtypes):
            if "*" in d:
                assert a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)), (name, d)
            else:
                assert a is ctype[d.split()[0]], (name, d)
    assert '#include "nnc_cbgrad_h16.h"' in open(os.path.join(ROOT, "include", "nnc.h")).read()
    assert nat.CBGRAD_H16_PLAN_LEN == len(nat.CBDX_H16_PLAN_FIELDS) == len(nat.CBDC_H16_PLAN_FIELDS) == 13


SHAPES = [(1, 37, 208), (7, 1000, 3000), (16, 4096, 4096), (17, 100, 100), (40, 100, 300), (130, 33, 129), (200, 1, 513), (512, 784, 300),
          (512, 4096, 4096), (4096, 4096, 4096), (4096, 5000, 5000), (100000, 70, 129), (64, 130, 100000)]


@pytest.mark.parametrize("dtype", h16_ref.DTYPES)
@pytest.mark.parametrize("lb,k", [(1, 256), (2, 257), (2, 1040)])
@pytest.mark.parametrize("m,kdim,ncols", SHAPES)
def test_plans_are_consistent_over_cu_counts(lib, m, kdim, ncols, lb, k, dtype):
    """splits independent of cus, per-split counts multiples of 32 on the MFMA path, workspace equal to the query, the split rule"""
    dx = [ops.cbmm_dx_h16_plan(TDT[dtype], m, kdim, ncols, lb, k, cus) for cus in CUS]
    dc = [ops.cbmm_dc_h16_plan(TDT[dtype], m, kdim, ncols, lb, k, cus) for cus in CUS]
    for plans, extent, per, query in ((dx, ncols, "cps", lib.nnc_cbmm_dx_h16_workspace_bytes(m, kdim, ncols, lb)),
                                      (dc, m, "rps", lib.nnc_cbmm_dc_h16_workspace_bytes(m, kdim, ncols, lb, k))):
        assert len({(p["splits"], p[per], p["workspace"], p["path"], p["lds"]) for p in plans}) == 1
        p = plans[0]
        assert p["workspace"] == query and p["dtype"] == h16_ref.DT_CODE[dtype]
        if m > 16:
            assert p["path"] == h16_ref.PATH_MFMA and p[per] % 32 == 0 and (p["splits"] - 1) * p[per] < extent <= p["splits"] * p[per]
            tiles = p["col_tiles"] * p["row_tiles"]
            assert p["splits"] <= max(1, min(-(-512 // tiles), extent // 64, 16))
            assert p["lds"] <= 64 * 1024
            assert all(q["col_tiles"] == p["col_tiles"] and q["row_tiles"] == p["row_tiles"] for q in plans)   # cus changes nothing here
        else:
            assert p["path"] == h16_ref.PATH_STREAM
    assert dx[0]["workspace"] == (dx[0]["splits"] * m * kdim * 4 if dx[0]["splits"] > 1 else 0)
    assert dc[0]["workspace"] == 64 + 8 * k
    if m > 16:
        assert dx[0]["col_tiles"] == -(-kdim // 128) and dx[0]["row_tiles"] == -(-m // 128)
        assert dc[0]["col_tiles"] == -(-ncols // 128) and dc[0]["row_tiles"] == -(-kdim // 128)
        assert 2 ** dc[0]["terms_log2"] >= kdim * ncols * dc[0]["splits"] > 2 ** (dc[0]["terms_log2"] - 1)


@pytest.mark.parametrize("dtype", h16_ref.DTYPES)
def test_stream_plans_are_the_float32_plans(lib, dtype):
    for m in (1, 2, 3, 5, 8, 9, 16):
        for kdim, ncols in ((37, 208), (129, 700), (40, 1000), (1, 77), (4096, 4096)):
            for lb, k in ((1, 200), (2, 257), (2, 1040)):
                for cus in (1, 80, 256, 304):
                    for addr in (0, 1, 4, 16):
                        a = ops.cbmm_dx_plan(m, kdim, ncols, lb, k, cus, addr * lb)
                        b = ops.cbmm_dx_h16_plan(TDT[dtype], m, kdim, ncols, lb, k, cus, addr * lb)
                        assert all(b[f] == v for f, v in a.items())
                        a = ops.cbmm_dc_plan(m, kdim, ncols, lb, k, cus, addr * lb)
                        b = ops.cbmm_dc_h16_plan(TDT[dtype], m, kdim, ncols, lb, k, cus, addr * lb)
                        assert all(b[f] == v for f, v in a.items())


@pytest.mark.parametrize("cus", [80, 256, 304])
def test_cases_cover_every_regime(lib, cus):
    dxs, dcs = set(), set()
    for case in href.CASES:
        _, m, kdim, ncols, lb, k, off, _ = case[0]
        for dtype in h16_ref.DTYPES:
            dxs.add(href.regime_of(case, ops.cbmm_dx_h16_plan(TDT[dtype], m, kdim, ncols, lb, k, cus, 256 + off * lb), dtype))
            dcs.add(href.regime_of(case, ops.cbmm_dc_h16_plan(TDT[dtype], m, kdim, ncols, lb, k, cus, 256 + off * lb), dtype))
    assert href.required_regimes("dx") <= dxs, href.required_regimes("dx") - dxs
    assert href.required_regimes("dc") <= dcs, href.required_regimes("dc") - dcs
    arms = {href.xvec_arms(c) for c in href.FULL if c[0][1] > 16}
    assert {a[0] for a in arms} == {True, False} and {a[1] for a in arms} == {True, False}
    # tails in both tile dimensions and two tiles, an m-split of dc: the shape the issue names
    p = ops.cbmm_dc_h16_plan(torch.bfloat16, 130, 33, 129, 1, 200, cus)
    assert p["splits"] == 2 and p["col_tiles"] == 2


@pytest.mark.parametrize("m,kdim,ncols,ax,ag", [(1 << 23, 1 << 20, 1 << 20, 65504.0, 65504.0), (17, 1 << 27, 1 << 27, 3.0e38, 1.0),
                                                (1 << 30, 128, 128, 1e-30, 1e-8), (4096, 4096, 4096, 1.0, 1.0), (1 << 40, 1, 1, 2.0 ** -24, 2.0 ** -24)])
def test_the_bound_keeps_the_integer_sums_in_int64(lib, m, kdim, ncols, ax, ag):
    """T and ops.cbgrad_shift at the extreme shapes: terms * |dW| 2^S < 2^62 whatever the data, in exact rational arithmetic"""
    for dtype in h16_ref.DTYPES:
        p = ops.cbmm_dc_h16_plan(TDT[dtype], m, kdim, ncols, 2, 1040, 256)
        T = p["terms_log2"]
        assert 2 ** T >= kdim * ncols * p["splits"] and T <= 62
        S, flag = ops.cbgrad_shift(m, ax, ag, T)
        if flag != ops.CBGRAD_OK:
            continue
        dw = Fraction(m) * Fraction(ax) * Fraction(ag)                      # the largest |dW| of a split
        total = kdim * ncols * p["splits"] * (dw * Fraction(2) ** S + Fraction(1, 2))
        assert total < 2 ** 62 + 2 ** T


def dx_call(lib, g=P, dt=1, m=4, kdim=8, labels=P, lb=1, ncols=16, centers=P, k=16, dx=P, dx_dt=0, ws=None, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbmm_dx_h16_workspace_bytes(m, kdim, ncols, lb) if min(m, kdim, ncols) >= 0 else 0
    return lib.nnc_cbmm_dx_h16(g, dt, m, kdim, labels, lb, ncols, centers, k, dx, dx_dt, ws, ws_bytes, None)


def dc_call(lib, x=P, g=P, dt=2, m=4, kdim=8, labels=P, lb=1, ncols=16, k=16, dc=P, f64=1, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbmm_dc_h16_workspace_bytes(m, kdim, ncols, lb, k) if min(m, kdim, ncols) >= 0 and 1 <= k <= 1040 else 0
    return lib.nnc_cbmm_dc_h16(x, g, dt, m, kdim, labels, lb, ncols, k, dc, f64, ws, ws_bytes, None)


BAD = [dict(m=-1), dict(kdim=-1), dict(ncols=-1), dict(k=0), dict(k=-3), dict(k=1041, lb=2), dict(lb=0), dict(lb=3),
       dict(k=257, lb=1), dict(k=1040, lb=1), dict(labels=None), dict(g=None), dict(ws_bytes=-1), dict(m=1 << 41),
       dict(dt=0), dict(dt=3), dict(dt=-1), dict(g=P + 1), dict(labels=P + 1, lb=2, k=300)]


@pytest.mark.parametrize("kw", BAD + [dict(centers=None), dict(dx=None), dict(dx_dt=2), dict(dx_dt=3), dict(dx=P + 2), dict(dx=P + 1, dx_dt=1),
                                      dict(m=40, ncols=300, ws=None), dict(m=40, ncols=300, ws=P + 2)])
def test_dx_bad_arguments_are_einval_without_a_device(lib, kw):
    assert dx_call(lib, **kw) == NNC_EINVAL
    assert lib.nnc_last_error()


@pytest.mark.parametrize("kw", BAD + [dict(x=None), dict(x=P + 1), dict(dc=None), dict(ws=None), dict(ws=P + 4)])
def test_dc_bad_arguments_are_einval_without_a_device(lib, kw):
    assert dc_call(lib, **kw) == NNC_EINVAL
    assert lib.nnc_last_error()


def test_short_workspace_is_enospace_without_a_device(lib):
    need = lib.nnc_cbmm_dx_h16_workspace_bytes(40, 100, 300, 2)
    assert need == 4 * 40 * 100 * 4
    assert dx_call(lib, m=40, kdim=100, ncols=300, lb=2, k=300, ws=P, ws_bytes=need - 1) == NNC_ENOSPACE
    need = lib.nnc_cbmm_dc_h16_workspace_bytes(40, 100, 300, 2, 300)
    assert need == 64 + 8 * 300
    assert dc_call(lib, m=40, kdim=100, ncols=300, lb=2, k=300, ws_bytes=need - 1) == NNC_ENOSPACE
    assert dc_call(lib, m=4, ws_bytes=0) == NNC_ENOSPACE
    assert lib.nnc_cbmm_dx_h16_workspace_bytes(-1, 1, 1, 1) == 0 and lib.nnc_cbmm_dc_h16_workspace_bytes(1, 1, 1, 3, 1) == 0


def test_huge_products_are_einval(lib):
    assert dx_call(lib, m=1, kdim=1 << 32, ncols=1 << 32) == NNC_EINVAL
    assert dc_call(lib, m=1, kdim=1 << 32, ncols=1 << 32) == NNC_EINVAL


@pytest.mark.parametrize("plan", ["nnc_cbmm_dx_h16_plan", "nnc_cbmm_dc_h16_plan"])
def test_plan_argument_errors_and_empty_shapes(lib, plan):
    fn = getattr(lib, plan)
    out = (ctypes.c_int64 * 13)()
    assert fn(1, 4, 8, 16, 1, 16, 0, 0, out) == NNC_EINVAL            # cus < 1
    assert fn(1, 4, 8, 16, 1, 16, 256, 0, None) == NNC_EINVAL         # out NULL
    assert fn(0, 4, 8, 16, 1, 16, 256, 0, out) == NNC_EINVAL          # float32 is not a dtype of this entry point
    assert fn(1, 4, 8, 16, 1, 257, 256, 0, out) == NNC_EINVAL
    assert fn(2, -1, 8, 16, 1, 16, 256, 0, out) == NNC_EINVAL
    for m, kdim, ncols in ((0, 50, 60), (4, 0, 60), (4, 50, 0), (20, 50, 0)):
        assert fn(2, m, kdim, ncols, 1, 8, 256, 0, out) == 0
        want = href.PATH_ZERO if plan.endswith("dc_h16_plan") or (m and kdim) else href.PATH_NONE
        assert out[0] == want and out[11] == 0 and out[12] == 2


def test_python_errors_that_need_no_device():
    with pytest.raises(TypeError):
        ops.cbmm_dx_h16_plan(torch.float32, 4, 8, 16, 1, 16, 256)
    with pytest.raises(TypeError):
        ops.cbmm_dc_h16_plan(torch.float64, 4, 8, 16, 1, 16, 256)
    g = torch.zeros(3, 16, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="CUDA"):                                     # a half tensor is still refused off the device
        ops.codebook_matmul_dx(g, torch.zeros(128, dtype=torch.uint8), torch.zeros(4), 8, 16)
    for kw in (dict(sparse=True), dict(sparse="auto"), dict(packed=True), dict(packed="auto")):
        with pytest.raises(ValueError, match="half_inputs"):
            compressed.compress_network_trainable(torch.nn.Module(), {}, half_inputs=True, **kw)
    with pytest.raises(ValueError, match="half_inputs"):
        compressed.compress_network(torch.nn.Module(), {}, half_inputs=True)          # not trainable
    with pytest.raises(ValueError, match="half_inputs"):
        compressed.compress_network(torch.nn.Module(), {}, trainable=True, half_inputs=True, sparse=True)
    assert "half_inputs" in compressed.TrainableCompressedDense.__init__.__code__.co_varnames
    assert "half_inputs" in compressed.TrainableCompressedConv2D.__init__.__code__.co_varnames
    import inspect

    from neural_network_compression_amd.common import trainer

    assert inspect.signature(trainer.Trainer.fine_tune_compressed).parameters["activation_dtype"].default is None
    assert not hasattr(compressed.TrainableGroupedCompressedDense, "half_inputs")     # grouped layers keep refusing
