"""CPU checks of the codebook backward pass's C ABI (include/nnc.h, nnc_cbmm_dx_* / nnc_cbmm_dc_*): the symbols, the argument
errors (returned before any HIP call, so none of this needs a device), the plans over CU counts, and the fixed-point shift rule
of the centroid gradient against its host mirror (ops.cbgrad_shift)."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from neural_network_compression_amd import compressed, ops
from tests.helpers import cbgrad_ref as ref

NNC_EINVAL, NNC_ENOSPACE = -1, -2
SYMBOLS = ("nnc_cbmm_dx_workspace_bytes", "nnc_cbmm_dx_plan", "nnc_cbmm_dx_f32",
           "nnc_cbmm_dc_workspace_bytes", "nnc_cbmm_dc_plan", "nnc_cbmm_dc_f32")
P = 0x1000   # a fake, never dereferenced address


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_symbols_are_exported_and_bound(lib):
    raw = ctypes.CDLL(nat.lib_path())
    for s in SYMBOLS:
        assert hasattr(raw, s) and s in nat.SIGNATURES
    assert nat.CBDX_PLAN_LEN == len(nat.CBDX_PLAN_FIELDS) and nat.CBDC_PLAN_LEN == len(nat.CBDC_PLAN_FIELDS)


def dx_call(lib, g=P, m=4, kdim=8, labels=P, lb=1, ncols=16, centers=P, k=16, dx=P, ws=None, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbmm_dx_workspace_bytes(m, kdim, ncols, lb) if min(m, kdim, ncols) >= 0 else 0
    return lib.nnc_cbmm_dx_f32(g, m, kdim, labels, lb, ncols, centers, k, dx, ws, ws_bytes, None)


def dc_call(lib, x=P, g=P, m=4, kdim=8, labels=P, lb=1, ncols=16, k=16, dc=P, f64=1, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbmm_dc_workspace_bytes(m, kdim, ncols, lb, k) if min(m, kdim, ncols) >= 0 and 1 <= k <= 1040 else 0
    return lib.nnc_cbmm_dc_f32(x, g, m, kdim, labels, lb, ncols, k, dc, f64, ws, ws_bytes, None)


BAD = [dict(m=-1), dict(kdim=-1), dict(ncols=-1), dict(k=0), dict(k=-3), dict(k=1041, lb=2), dict(lb=0), dict(lb=3),
       dict(k=257, lb=1), dict(k=1040, lb=1), dict(labels=None), dict(g=None), dict(ws_bytes=-1), dict(m=1 << 41)]


@pytest.mark.parametrize("kw", BAD + [dict(centers=None), dict(dx=None)])
def test_dx_bad_arguments_are_einval_without_a_device(lib, kw):
    assert dx_call(lib, **kw) == NNC_EINVAL
    assert lib.nnc_last_error()


@pytest.mark.parametrize("kw", BAD + [dict(x=None), dict(dc=None), dict(ws=None), dict(ws=P + 4)])
def test_dc_bad_arguments_are_einval_without_a_device(lib, kw):
    assert dc_call(lib, **kw) == NNC_EINVAL
    assert lib.nnc_last_error()


def test_short_workspace_is_enospace_without_a_device(lib):
    need = lib.nnc_cbmm_dx_workspace_bytes(1, 5000, 5000, 1)
    assert need > 0                                           # the 25 M-weight layer at m = 1 splits ncols
    assert dx_call(lib, m=1, kdim=5000, ncols=5000, ws=P, ws_bytes=need - 1) == NNC_ENOSPACE
    assert dx_call(lib, m=1, kdim=5000, ncols=5000, ws=None, ws_bytes=need) == NNC_EINVAL
    need = lib.nnc_cbmm_dc_workspace_bytes(1, 5000, 5000, 2, 1040)
    assert need == 64 + 8 * 1040
    assert dc_call(lib, m=1, kdim=5000, ncols=5000, lb=2, k=1040, ws_bytes=need - 1) == NNC_ENOSPACE


def test_huge_products_are_einval(lib):
    assert dc_call(lib, m=4, kdim=1 << 30, ncols=1 << 30, ws_bytes=1 << 20) == NNC_EINVAL
    out = (ctypes.c_int64 * nat.CBDC_PLAN_LEN)()
    assert lib.nnc_cbmm_dc_plan(4, 1 << 30, 1 << 30, 1, 16, 256, 0, out) == NNC_EINVAL


@pytest.mark.parametrize("plan", [ops.cbmm_dx_plan, ops.cbmm_dc_plan])
def test_plan_argument_errors(lib, plan):
    with pytest.raises(nat.NncError):
        plan(4, 8, 16, 1, 16, 0)
    with pytest.raises(nat.NncError):
        plan(4, 8, 16, 1, 300, 64)
    out_null = lib.nnc_cbmm_dx_plan(4, 8, 16, 1, 16, 64, 0, None)
    assert out_null == NNC_EINVAL


SHAPES = [(1, 1, 1), (1, 5000, 5000), (3, 17, 65), (16, 784, 300), (16, 8192, 8192), (17, 100, 100), (40, 100, 300),
          (256, 5000, 5000), (256, 100, 70), (4096, 2450, 256), (4096, 5000, 5000), (100000, 300, 100), (2, 1, 77)]


@pytest.mark.parametrize("m,kdim,ncols", SHAPES)
@pytest.mark.parametrize("lb,k", [(1, 256), (2, 257), (2, 1040), (1, 1)])
def test_plans_are_consistent_over_cu_counts(lib, m, kdim, ncols, lb, k):
    dx_ref = dc_ref = None
    for cus in list(range(1, 17)) + [31, 64, 100, 128, 255, 256, 257, 304, 511, 512]:
        for addr in (0, 1, 3):
            dx = ops.cbmm_dx_plan(m, kdim, ncols, lb, k, cus, addr * lb)
            dc = ops.cbmm_dc_plan(m, kdim, ncols, lb, k, cus, addr * lb)
            # the splits (so the bits of dx and dc) and the workspace depend on the shape alone
            key_dx = (dx["path"], dx["splits"], dx["cps"], dx["workspace"])
            key_dc = (dc["path"], dc["splits"], dc["rps"], dc["terms_log2"], dc["workspace"])
            dx_ref = dx_ref or key_dx
            dc_ref = dc_ref or key_dc
            assert key_dx == dx_ref and key_dc == dc_ref
            assert dx["workspace"] == lib.nnc_cbmm_dx_workspace_bytes(m, kdim, ncols, lb)
            assert dc["workspace"] == lib.nnc_cbmm_dc_workspace_bytes(m, kdim, ncols, lb, k)
            if m <= 16:
                assert dx["path"] == dc["path"] == ref.PATH_STREAM
                e = dx["vb"] // lb
                assert dx["mt"] >= m and dx["mt"] * e <= 64 and dx["col_tiles"] * 64 * e >= ncols > (dx["col_tiles"] - 1) * 64 * e
                assert dx["splits"] == dx["col_tiles"] and dc["splits"] == 1
                assert 1 <= dx["row_tiles"] <= max(1, 2 * min(cus, 256)) and dx["row_tiles"] <= kdim
                assert dx["copies"] * dx["entries"] * 4 + dx["entries"] * 4 == dx["lds"] <= 64 * 1024
                assert dx["entries"] == (256 if lb == 1 else k + 1)
                assert dx["aligned"] == int(addr == 0 and (ncols * lb) % dx["vb"] == 0)
            else:
                assert dx["path"] == dc["path"] == ref.PATH_TILED
                assert dx["col_tiles"] * 128 >= kdim and dx["row_tiles"] * 128 >= m
                assert dc["col_tiles"] * 128 >= ncols and dc["row_tiles"] * 128 >= kdim
                assert 1 <= dx["splits"] <= 16 and dx["splits"] * dx["cps"] >= ncols > (dx["splits"] - 1) * dx["cps"]
                assert 1 <= dc["splits"] <= 16 and dc["splits"] * dc["rps"] >= m > (dc["splits"] - 1) * dc["rps"]
            assert dc["terms_log2"] == math.ceil(math.log2(kdim * ncols * dc["splits"]))
            assert dc["lds"] <= 64 * 1024
            assert dx["workspace"] == (dx["splits"] * m * kdim * 4 if dx["splits"] > 1 else 0)


@pytest.mark.parametrize("m,kdim,ncols,dxp,dcp", [(0, 5, 5, ref.PATH_NONE, ref.PATH_ZERO), (3, 0, 5, ref.PATH_NONE, ref.PATH_ZERO),
                                                  (3, 5, 0, ref.PATH_ZERO, ref.PATH_ZERO), (30, 5, 0, ref.PATH_ZERO, ref.PATH_ZERO)])
def test_empty_shapes_plan(lib, m, kdim, ncols, dxp, dcp):
    assert ops.cbmm_dx_plan(m, kdim, ncols, 1, 4, 256)["path"] == dxp
    assert ops.cbmm_dc_plan(m, kdim, ncols, 1, 4, 256)["path"] == dcp
    assert lib.nnc_cbmm_dx_workspace_bytes(m, kdim, ncols, 1) == 0 and lib.nnc_cbmm_dc_workspace_bytes(m, kdim, ncols, 1, 4) == 0


def test_regime_cases_cover_every_regime(lib):
    for cus in (1, 32, 256, 304):
        dxs, dcs = set(), set()
        for case in ref.REGIME_CASES:
            _, m, kdim, ncols, lb, k, off, _ = case
            dxs.add(ref.dx_regime(ops.cbmm_dx_plan(m, kdim, ncols, lb, k, cus, 256 + off * lb)))
            dcs.add(ref.dc_regime(ops.cbmm_dc_plan(m, kdim, ncols, lb, k, cus, 256 + off * lb)))
        assert ref.DX_REQUIRED <= dxs, ref.DX_REQUIRED - dxs
        assert ref.DC_REQUIRED <= dcs, ref.DC_REQUIRED - dcs


def _shift_rule(m, ax, ag, t):
    """include/nnc.h in exact rational arithmetic: S = 62 - T - P with P the least integer such that 2^P > fl64(fl64(m * ax) * ag)."""
    bound = float(m) * float(np.float32(ax)) * float(np.float32(ag))
    if bound == 0:
        return None
    b = Fraction(bound)
    P = math.floor(math.log2(bound)) - 2
    while Fraction(2) ** P <= b:
        P += 1
    return 62 - t - P


@pytest.mark.parametrize("seed", range(4))
def test_shift_mirror_matches_the_rule(seed):
    rng = np.random.RandomState(seed)
    for _ in range(500):
        m = int(rng.choice([1, 3, 16, 17, 256, 4096, 1 << 20]))
        ax = float(np.float32(np.ldexp(rng.rand() + 0.5, rng.randint(-60, 40))))
        ag = float(np.float32(np.ldexp(rng.rand() + 0.5, rng.randint(-60, 40))))
        t = int(rng.randint(0, 56))
        S, flag = ops.cbgrad_shift(m, ax, ag, t)
        assert flag == ops.CBGRAD_OK and S == _shift_rule(m, ax, ag, t)
    for ax in (1.0, 0.5, 2.0 ** -20, 3.0):                   # exact powers of two: 2^P must exceed the bound strictly
        S, _ = ops.cbgrad_shift(1, ax, 1.0, 0)
        assert 2.0 ** (62 - S) > ax and 2.0 ** (61 - S) <= ax
    assert ops.cbgrad_shift(4, 0.0, 1.0, 10) == (0, ops.CBGRAD_ZERO)
    assert ops.cbgrad_shift(4, float("inf"), 1.0, 10) == (0, ops.CBGRAD_NONFINITE)
    assert ops.cbgrad_shift(4, 1.0, float("nan"), 10) == (0, ops.CBGRAD_NONFINITE)
    assert ops.cbgrad_shift(1 << 20, 3e38, 3e38, 10)[1] == ops.CBGRAD_NONFINITE   # P > 127


@pytest.mark.parametrize("m,kdim,ncols", [(1, 1, 1), (16, 5000, 5000), (1 << 40, 1, 1), (4096, 1 << 27, 1 << 28), (1 << 20, 1 << 20, 1 << 20 >> 6),
                                          (300, 8192, 8192)])
@pytest.mark.parametrize("ax,ag", [(1.0, 1.0), (3.4e38, 1e-30), (1e-30, 1e-30), (2.0 ** 60, 2.0 ** -3), (65504.0, 65504.0)])
def test_the_bound_keeps_the_integer_sums_in_int64(m, kdim, ncols, ax, ag):
    """Every image rint(dW 2^S) is at most 2^(P+S) (1 + u)^m and there are at most 2^T of them: |sum| < 2^62 (1 + u)^m."""
    lb, k = 2, 1040
    try:
        plan = ops.cbmm_dc_plan(m, kdim, ncols, lb, k, 256)
    except nat.NncError:
        assert kdim * ncols > (1 << 55) or max(m, kdim, ncols) > (1 << 40)
        return
    t = plan["terms_log2"]
    assert (1 << t) >= kdim * ncols * plan["splits"]
    S, flag = ops.cbgrad_shift(m, ax, ag, t)
    if flag != ops.CBGRAD_OK:
        return
    bound = Fraction(float(m) * float(np.float32(ax)) * float(np.float32(ag)))
    P = 62 - t - S
    assert Fraction(2) ** P > bound                                     # every float32 |dW| <= bound (1 + u)^m < 2^P (1 + u)^m
    assert (kdim * ncols * plan["splits"]) * Fraction(2) ** (P + S) <= Fraction(2) ** 62


def test_trainable_needs_the_dense_form():
    with pytest.raises(ValueError, match="sparse"):
        compressed.compress_network(None, {}, sparse=True, trainable=True)
    with pytest.raises(ValueError, match="sparse"):
        compressed.compress_network(None, {}, sparse="auto", trainable=True)


def test_centroid_grad_takes_a_non_finite_flag_and_checks_its_arguments(lib):
    """nnc_centroid_grad_f32 (the backward of a quantized bias and of Trainer.fine_tune_centroids): the non-finite flag word is a
    required argument; argument errors come before any HIP call."""
    assert len(nat.SIGNATURES["nnc_centroid_grad_f32"][1]) == 10
    ok = dict(grad=P, labels=P, lb=1, n=10, k=4, S=0, sums=P, counts=0, nonfinite=P)
    assert lib.nnc_centroid_grad_f32(*(dict(ok, nonfinite=0).values()), None) == NNC_EINVAL
    for bad in (dict(sums=0), dict(k=0), dict(lb=3), dict(n=-1), dict(grad=0), dict(labels=0)):
        assert lib.nnc_centroid_grad_f32(*(dict(ok, **bad).values()), None) == NNC_EINVAL, bad
