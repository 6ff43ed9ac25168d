"""CPU checks of the C ABI of the half-precision bitmap-sparse codebook backward pass (include/nnc_cbspgrad_h16.h, nnc_cbsp_dx_h16 /
nnc_cbsp_dc_h16): the header against the bound signatures, the plan equalities over CU counts (m <= 16: the
float32 sparse plans field for field; m > 16: the byte form's half plans in every shared field), the regimes the case list of
tests/helpers/sparse_h16_grad_ref.py hits, the fixed-point bounds at the extreme shapes (the int64 sums, and the per-lane register
of the skipped weights of k_cbspdc_mfma) in exact rational arithmetic, every argument error (returned before any HIP call, so none
of this needs a device) and the Python errors that need none."""
import ctypes
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from neural_network_compression_amd import compressed, ops
from neural_network_compression_amd.common import trainer
from tests.helpers import cbgrad_ref, h16_ref
from tests.helpers import sparse_h16_grad_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NNC_EINVAL, NNC_ENOSPACE = -1, -2
P = 0x1000   # a fake, never dereferenced, 256-byte aligned address
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
CUS = (1, 80, 256, 1024)


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_symbols_header_and_signatures_agree(lib):
    """every prototype of include/nnc_cbspgrad_h16.h is exported and bound with the arguments it declares, from a table of its own;
    nnc.h includes the header"""
    text = open(os.path.join(ROOT, "include", "nnc_cbspgrad_h16.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(int64_t|int)\s+(nnc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    assert {p[1] for p in protos} == set(nat.SPARSE_H16_GRAD_SIGNATURES) and len(protos) == 6
    assert {p[1] for p in protos} == {f"nnc_cbsp_{d}_h16{s}" for d in ("dx", "dc") for s in ("_workspace_bytes", "_plan", "")}
    assert not set(nat.SPARSE_H16_GRAD_SIGNATURES) & set(nat.SIGNATURES)
    raw = ctypes.CDLL(nat.lib_path())
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64}
    for ret, name, args in protos:
        res, argtypes = nat.SPARSE_H16_GRAD_SIGNATURES[name]
        assert hasattr(raw, name) and res is ctype[ret]
        decl = [a.strip() for a in args.split(",")]
        assert len(decl) == len(argtypes), name
        for d, a in zip(decl, argtypes):
            if "*" in d:
                assert a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)), (name, d)
            else:
                assert a is ctype[d.split()[0]], (name, d)
    assert '#include "nnc_cbspgrad_h16.h"' in open(os.path.join(ROOT, "include", "nnc.h")).read()
    assert nat.CBSPGRAD_H16_PLAN_LEN == len(nat.CBSPDX_H16_PLAN_FIELDS) == len(nat.CBSPDC_H16_PLAN_FIELDS) == 12
    assert nat.CBSPDX_H16_PLAN_FIELDS[:-1] == nat.CBSPDX_PLAN_FIELDS and nat.CBSPDC_H16_PLAN_FIELDS[:-1] == nat.CBSPDC_PLAN_FIELDS


SHAPES = [(1, 37, 208), (7, 1000, 3000), (16, 4096, 4096), (16, 5000, 5000), (17, 100, 100), (40, 100, 330), (130, 33, 129), (200, 1, 513),
          (512, 784, 300), (512, 4096, 4096), (4096, 5000, 5000), (100000, 70, 129), (64, 130, 100000)]
DX_SHARED = ("path", "mt", "copies", "entries", "splits", "cps", "lds", "col_tiles", "row_tiles", "workspace", "dtype")
DC_SHARED = ("path", "mt", "copies", "splits", "rps", "lds", "col_tiles", "row_tiles", "terms_log2", "workspace", "dtype")


@pytest.mark.parametrize("dtype", h16_ref.DTYPES)
@pytest.mark.parametrize("lb,k", [(1, 256), (2, 257), (2, 1040)])
@pytest.mark.parametrize("m,kdim,ncols", SHAPES)
def test_plans_equal_the_plans_they_follow(lib, m, kdim, ncols, lb, k, dtype):
    """m <= 16: nnc_cbsp_dx_plan / nnc_cbsp_dc_plan field for field.  m > 16: every field shared with nnc_cbmm_dx_h16_plan /
    nnc_cbmm_dc_h16_plan (tiles, splits, per-split extent, LDS, TERMS_LOG2, workspace), PATH = NNC_CBMM_MFMA.  At 1, 80, 256 and 1024
    CUs; the splits depend on the shape alone (planned for 256 CUs) and never shrink with more; the workspace is the query's."""
    t = TDT[dtype]
    dxs = [ops.cbsp_dx_h16_plan(t, m, kdim, ncols, lb, k, cus) for cus in CUS]
    dcs = [ops.cbsp_dc_h16_plan(t, m, kdim, ncols, lb, k, cus) for cus in CUS]
    for cus, dx, dc in zip(CUS, dxs, dcs):
        assert dx["dtype"] == dc["dtype"] == h16_ref.DT_CODE[dtype]
        if m <= 16:
            a, b = ops.cbsp_dx_plan(m, kdim, ncols, lb, k, cus), ops.cbsp_dc_plan(m, kdim, ncols, lb, k, cus)
            assert all(dx[f] == v for f, v in a.items()) and all(dc[f] == v for f, v in b.items())
            assert dx["path"] == dc["path"] == h16_ref.PATH_STREAM
        else:
            a, b = ops.cbmm_dx_h16_plan(t, m, kdim, ncols, lb, k, cus), ops.cbmm_dc_h16_plan(t, m, kdim, ncols, lb, k, cus)
            assert all(dx[f] == a[f] for f in DX_SHARED) and all(dc[f] == b[f] for f in DC_SHARED)
            assert dx["path"] == dc["path"] == h16_ref.PATH_MFMA and dx["segs"] == dc["segs"] == 0
            assert dx["cps"] % 32 == 0 and dc["rps"] % 32 == 0
    assert len({(p["splits"], p["cps"], p["workspace"], p["path"]) for p in dxs}) == 1
    assert len({(p["splits"], p["rps"], p["workspace"], p["path"], p["terms_log2"], p["copies"]) for p in dcs}) == 1
    assert dxs[0]["workspace"] == lib.nnc_cbsp_dx_h16_workspace_bytes(m, kdim, ncols, lb)
    assert dcs[0]["workspace"] == lib.nnc_cbsp_dc_h16_workspace_bytes(m, kdim, ncols, lb, k) == 64 + 8 * k
    # the splits of dc, its bin copies and T are the byte form's half plan's at every m: S and the images are that call's
    b = ops.cbmm_dc_h16_plan(t, m, kdim, ncols, lb, k, 256)
    assert all(dcs[0][f] == b[f] for f in ("splits", "rps", "copies", "terms_log2"))


@pytest.mark.parametrize("cus", [80, 256])
def test_cases_cover_every_regime(lib, cus):
    dxs, dcs = set(), set()
    for c in sref.CASES:
        for dtype in h16_ref.DTYPES:
            dxs.add(sref.regime_of(c, ops.cbsp_dx_h16_plan(TDT[dtype], c["m"], c["kdim"], c["ncols"], c["lb"], c["k"], cus), dtype))
            dcs.add(sref.regime_of(c, ops.cbsp_dc_h16_plan(TDT[dtype], c["m"], c["kdim"], c["ncols"], c["lb"], c["k"], cus), dtype))
    assert sref.required_regimes("dx") <= dxs, sref.required_regimes("dx") - dxs
    assert sref.required_regimes("dc") <= dcs, sref.required_regimes("dc") - dcs
    arms = {sref.xvec_arms(c) for c in sref.CASES if c["m"] > 16}
    assert {a[0] for a in arms} == {True, False} and {a[1] for a in arms} == {True, False}
    assert {c["z"] for c in sref.CASES} == set(sref.Z_KINDS) and any(c["beyond"] for c in sref.CASES) and any(c["density"] == 0 for c in sref.CASES)
    assert {c["k"] for c in sref.CASES} >= {1, 2, 256, 257}
    # a split of ncols that cuts a bitmap word in two (a multiple of 32 that is no multiple of 64), and a split of m in dc
    assert any(ops.cbsp_dx_h16_plan(torch.bfloat16, c["m"], c["kdim"], c["ncols"], c["lb"], c["k"], cus)["cps"] % 64 == 32 for c in sref.CASES if c["m"] > 16)
    assert any(ops.cbsp_dc_h16_plan(torch.bfloat16, c["m"], c["kdim"], c["ncols"], c["lb"], c["k"], cus)["splits"] > 1 for c in sref.CASES)


EXTREME = [(1 << 23, 1 << 20, 1 << 20, 65504.0, 65504.0), (17, 1 << 34, 64, 3.0e38, 1.0), (1 << 30, 128, 128, 1e-30, 1e-8), (4096, 4096, 4096, 1.0, 1.0),
           (1 << 40, 1, 1, 2.0 ** -24, 2.0 ** -24), (17, 1, 1, 1.0, 1.0), (300, 3, 5, 7.0, 0.5), (33, 1, 63, 65504.0, 65504.0)]


@pytest.mark.parametrize("m,kdim,ncols,ax,ag", EXTREME)
def test_the_bounds_keep_the_integer_sums_and_the_skipped_register_in_int64(lib, m, kdim, ncols, ax, ag):
    """T and ops.cbgrad_shift at the extreme shapes, in exact rational arithmetic.  Every image rint(dW 2^S) is at most
    2^(P + S) (1 + u)^m in magnitude (+ 1/2 for the rounding) and there are at most 2^T of them: the int64 sums stay within 2^62 (1 +
    u)^m, section 12's bound.  The per-lane register of k_cbspdc_mfma for bin z holds the images of a subset of one lane's
    accumulators: 2 x 2 MFMA blocks of 16 registers, so at most min(64, kdim * ncols) of the terms of one split of m -- a subset of
    the 2^T terms, and also directly: 64 images of at most 2^(62 - T) (1 + u)^m each stay below 2^63 for every T >= 0 only because
    a lane has no more valid accumulators than the layer has positions; (1 + u)^m < 1.65 up to m = 2^23 (u = 2^-24)."""
    for dtype in h16_ref.DTYPES:
        p = ops.cbsp_dc_h16_plan(TDT[dtype], m, kdim, ncols, 2, 1040, 256)
        T = p["terms_log2"]
        assert 2 ** T >= kdim * ncols * p["splits"] and T <= 62
        S, flag = ops.cbgrad_shift(m, ax, ag, T)
        if flag != ops.CBGRAD_OK:
            continue
        bound = Fraction(float(m) * float(np.float32(ax)) * float(np.float32(ag)))
        Pexp = 62 - T - S
        assert Fraction(2) ** Pexp > bound
        image = Fraction(2) ** (Pexp + S)                                   # the largest image, but for (1 + u)^m and the rounding
        growth = Fraction(165, 100) if m <= 1 << 23 else None               # (1 + 2^-24)^(2^23) = 1.6487...
        if m <= 1 << 23:
            assert (1 + Fraction(1, 1 << 24)) ** min(m, 1 << 12) <= growth  # (spot check of the constant on a power that is cheap)
        assert kdim * ncols * p["splits"] * image <= Fraction(2) ** 62      # the sums: section 12's bound
        lane_terms = min(64, kdim * ncols)                                  # valid accumulators of one lane of one workgroup
        assert lane_terms <= kdim * ncols * p["splits"] <= 2 ** T
        reg = lane_terms * (image + Fraction(1, 2))
        assert reg <= Fraction(2) ** 62 + 32                                # before the growth factor
        if growth is not None:
            assert lane_terms * (image * growth + Fraction(1, 2)) < Fraction(2) ** 63


def dx_call(lib, g=P, dt=1, m=4, kdim=8, packed=P, packed_bytes=None, lb=1, ncols=16, z=0, nnz=5, centers=P, k=16, dx=P, dx_dt=0, ws=P, ws_bytes=None):
    if packed_bytes is None:
        packed_bytes = lib.nnc_cbsp_pack_bytes(kdim, ncols, lb, nnz) if min(kdim, ncols, nnz) >= 0 and lb in (1, 2) else 1 << 20
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbsp_dx_h16_workspace_bytes(m, kdim, ncols, lb) if min(m, kdim, ncols) >= 0 else 0
    return lib.nnc_cbsp_dx_h16(g, dt, m, kdim, packed, packed_bytes, lb, ncols, z, nnz, centers, k, dx, dx_dt, ws, ws_bytes, None)


def dc_call(lib, x=P, g=P, dt=2, m=4, kdim=8, packed=P, packed_bytes=None, lb=1, ncols=16, z=0, nnz=5, k=16, dc=P, f64=1, ws=P, ws_bytes=None):
    if packed_bytes is None:
        packed_bytes = lib.nnc_cbsp_pack_bytes(kdim, ncols, lb, nnz) if min(kdim, ncols, nnz) >= 0 and lb in (1, 2) else 1 << 20
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbsp_dc_h16_workspace_bytes(m, kdim, ncols, lb, k) if min(m, kdim, ncols) >= 0 and 1 <= k <= 1040 else 0
    return lib.nnc_cbsp_dc_h16(x, g, dt, m, kdim, packed, packed_bytes, lb, ncols, z, nnz, k, dc, f64, ws, ws_bytes, None)


# (arguments, a piece of the message): section 22's errors (the dtypes, the addresses) and section 13's (the sizes, the form)
BAD = [(dict(dt=0), "x_dtype must be NNC_DT_BF16 or NNC_DT_F16"), (dict(dt=3), "x_dtype"), (dict(dt=-1), "x_dtype"),
       (dict(m=-1), "negative size"), (dict(kdim=-1), "negative size"), (dict(ncols=-1), "negative size"),
       (dict(lb=0), "label_bytes must be 1 or 2"), (dict(lb=3), "label_bytes must be 1 or 2"),
       (dict(k=0), "k outside 1..NNC_KMAX"), (dict(k=1041, lb=2), "k outside 1..NNC_KMAX"), (dict(k=257, lb=1), "k > 256 needs 2-byte labels"),
       (dict(m=1 << 41), "size too large"), (dict(ncols=1 << 32, kdim=1), "size too large"), (dict(kdim=1 << 38, ncols=1 << 10), "size too large"),
       (dict(z=-1), "zero_symbol outside the label range"), (dict(z=256), "zero_symbol outside the label range"), (dict(z=65536, lb=2), "zero_symbol"),
       (dict(nnz=-1), "nnz outside 0..kdim * ncols"), (dict(nnz=129), "nnz outside 0..kdim * ncols"),
       (dict(packed_bytes=10), "packed buffer smaller than nnc_cbsp_pack_bytes"), (dict(packed=None), "packed is NULL"),
       (dict(packed=P + 128), "packed must be 256-byte aligned"), (dict(g=None), "is NULL"), (dict(g=P + 1), "not aligned to its element size"),
       (dict(ws_bytes=-1), "negative workspace size")]


@pytest.mark.parametrize("kw,msg", BAD + [(dict(centers=None), "centers is NULL"), (dict(dx=None), "dx is NULL"),
                                          (dict(dx_dt=2), "dx_dtype must be NNC_DT_F32 or x_dtype"), (dict(dx_dt=3), "dx_dtype"),
                                          (dict(dx=P + 2), "not aligned to its element size"), (dict(dx=P + 1, dx_dt=1), "not aligned to its element size"),
                                          (dict(ws=None), "workspace is NULL"), (dict(ws=P + 2), "workspace must be 4-byte aligned"),
                                          (dict(m=40, ncols=330, nnz=5, ws=None), "workspace is NULL")])
def test_dx_bad_arguments_are_einval_without_a_device(lib, kw, msg):
    assert dx_call(lib, **kw) == NNC_EINVAL
    err = lib.nnc_last_error().decode()
    assert err.startswith("nnc_cbsp_dx_h16: ") and msg in err, err


@pytest.mark.parametrize("kw,msg", BAD + [(dict(x=None), "x or g is NULL"), (dict(x=P + 1), "not aligned to its element size"), (dict(dc=None), "dc is NULL"),
                                          (dict(ws=None), "workspace is NULL"), (dict(ws=P + 4), "workspace not 8-byte aligned")])
def test_dc_bad_arguments_are_einval_without_a_device(lib, kw, msg):
    assert dc_call(lib, **kw) == NNC_EINVAL
    err = lib.nnc_last_error().decode()
    assert err.startswith("nnc_cbsp_dc_h16: ") and msg in err, err


def test_short_workspace_is_enospace_without_a_device(lib):
    need = lib.nnc_cbsp_dx_h16_workspace_bytes(40, 100, 330, 2)
    assert need == ops.cbmm_dx_h16_plan(torch.bfloat16, 40, 100, 330, 2, 300, 256)["workspace"] > 0
    assert dx_call(lib, m=40, kdim=100, ncols=330, lb=2, k=300, ws_bytes=need - 1) == NNC_ENOSPACE
    assert "workspace smaller than nnc_cbsp_dx_h16_workspace_bytes()" in lib.nnc_last_error().decode()
    need = lib.nnc_cbsp_dx_h16_workspace_bytes(4, 8, 16, 1)
    assert need == lib.nnc_cbsp_dx_workspace_bytes(4, 8, 16, 1) == 16                       # m <= 16: the row sums of g
    assert dx_call(lib, ws_bytes=need - 1) == NNC_ENOSPACE
    need = lib.nnc_cbsp_dc_h16_workspace_bytes(40, 100, 330, 2, 300)
    assert need == 64 + 8 * 300
    assert dc_call(lib, m=40, kdim=100, ncols=330, lb=2, k=300, ws_bytes=need - 1) == NNC_ENOSPACE
    assert "workspace smaller than nnc_cbsp_dc_h16_workspace_bytes()" in lib.nnc_last_error().decode()
    assert lib.nnc_cbsp_dx_h16_workspace_bytes(-1, 1, 1, 1) == 0 and lib.nnc_cbsp_dc_h16_workspace_bytes(1, 1, 1, 3, 1) == 0


@pytest.mark.parametrize("plan", ["nnc_cbsp_dx_h16_plan", "nnc_cbsp_dc_h16_plan"])
def test_plan_argument_errors_and_empty_shapes(lib, plan):
    fn = getattr(lib, plan)
    out = (ctypes.c_int64 * 12)()
    for args, msg in (((1, 4, 8, 16, 1, 16, 0, out), "cus < 1"), ((1, 4, 8, 16, 1, 16, 256, None), "out is NULL"),
                      ((0, 4, 8, 16, 1, 16, 256, out), "x_dtype must be NNC_DT_BF16 or NNC_DT_F16"),        # float32 is not a dtype of this entry point
                      ((1, 4, 8, 16, 1, 257, 256, out), "k > 256 needs 2-byte labels"), ((2, -1, 8, 16, 1, 16, 256, out), "negative size")):
        assert fn(*args) == NNC_EINVAL
        err = lib.nnc_last_error().decode()
        assert err.startswith(plan + ": ") and msg in err, err
    # empty shapes follow section 13: m = 0 or kdim = 0: dx is empty; ncols = 0: dx = 0; any empty dimension: dc = 0
    for m, kdim, ncols in ((0, 50, 60), (4, 0, 60), (4, 50, 0), (20, 50, 0), (0, 0, 0)):
        assert fn(2, m, kdim, ncols, 1, 8, 256, out) == 0
        f32 = (ops.cbsp_dc_plan if plan.endswith("dc_h16_plan") else ops.cbsp_dx_plan)(m, kdim, ncols, 1, 8, 256)
        assert list(out)[:11] == list(f32.values()) and out[11] == 2
        assert out[0] == (cbgrad_ref.PATH_NONE if "dx" in plan and not (m and kdim) else cbgrad_ref.PATH_ZERO) and out[10] == 0


def test_python_errors_that_need_no_device():
    with pytest.raises(TypeError):
        ops.cbsp_dx_h16_plan(torch.float32, 4, 8, 16, 1, 16, 256)
    with pytest.raises(TypeError):
        ops.cbsp_dc_h16_plan(torch.float64, 4, 8, 16, 1, 16, 256)
    g = torch.zeros(3, 16, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="CUDA"):                                     # a half tensor is still refused off the device
        ops.sparse_codebook_matmul_dx(g, None, torch.zeros(4))
    with pytest.raises(TypeError, match="one dtype"):
        ops.sparse_codebook_centroid_grad(torch.zeros(3, 8, dtype=torch.float16), g, None)
    with pytest.raises(TypeError, match="one dtype"):
        ops.sparse_codebook_centroid_grad(torch.zeros(3, 8), g, None)
    assert "ops.sparse_codebook_linear" in inspect.getsource(ops._require_f32_x) and "forward only" not in inspect.getsource(ops._require_f32_x)
    net = torch.nn.Module()
    for kw in (dict(sparse=False), dict(), dict(sparse=True, packed=True), dict(sparse="auto", packed="auto")):
        with pytest.raises(ValueError, match="sparse_half_inputs"):
            compressed.compress_network_trainable(net, {}, sparse_half_inputs=True, **kw)
    for kw in (dict(sparse=True), dict(sparse="auto")):                              # pinned: the byte option does not combine with sparse
        with pytest.raises(ValueError, match="half_inputs"):
            compressed.compress_network_trainable(net, {}, half_inputs=True, **kw)
        with pytest.raises(ValueError, match="compress_network_trainable"):
            compressed.compress_network(net, {}, trainable=True, sparse_half_inputs=True, **kw)
    assert inspect.signature(compressed.compress_network_trainable).parameters["sparse_half_inputs"].default is False
    assert inspect.signature(trainer.Trainer.fine_tune_compressed).parameters["sparse_half_inputs"].default is False


def test_fine_tune_compressed_keyword_errors_need_no_device():
    """sparse_half_inputs=True without activation_dtype, with sparse=False or with packed; activation_dtype with sparse and without the
    new keyword: ValueError, before anything is built"""
    class Bare(trainer.Trainer):   # the abstract parts are never reached: the keyword checks come first
        model_name = "bare"

        def _get_error(self, *a):
            raise AssertionError

        def _layers_to_prune_with_threshold(self, *a):
            raise AssertionError

    t = Bare.__new__(Bare)
    t.quantized_models_by_layer = {object(): [None, None]}
    for kw in (dict(sparse=True, sparse_half_inputs=True), dict(sparse=False, sparse_half_inputs=True, activation_dtype=torch.bfloat16),
               dict(sparse=True, packed=True, sparse_half_inputs=True, activation_dtype=torch.float16)):
        with pytest.raises(ValueError, match="sparse_half_inputs"):
            t.fine_tune_compressed(None, None, epochs=1, **kw)
    for kw in (dict(sparse=True), dict(sparse="auto")):
        with pytest.raises(ValueError, match="sparse_half_inputs"):
            t.fine_tune_compressed(None, None, epochs=1, activation_dtype=torch.bfloat16, **kw)
    with pytest.raises(ValueError, match="activation_dtype"):
        t.fine_tune_compressed(None, None, epochs=1, activation_dtype=torch.float64, sparse=True, sparse_half_inputs=True)


def test_layer_signatures():
    """half_inputs is the last keyword, default False, of the constructors and of from_dense / from_conv; both from_codes signatures
    are what they were"""
    for fn in (compressed._TrainableSparseCodebookLayer.__init__, compressed.TrainableSparseCompressedDense.__init__,
               compressed.TrainableSparseCompressedConv2D.__init__, compressed.TrainableSparseCompressedDense.from_dense,
               compressed.TrainableSparseCompressedConv2D.from_conv):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "half_inputs" and params[-1].default is False, fn
    assert list(inspect.signature(compressed.TrainableSparseCompressedDense.from_codes).parameters) == \
        ["kdim", "ncols", "labels", "centers", "bias", "bias_codes", "activation", "zero_symbol"]
    assert list(inspect.signature(compressed.TrainableSparseCompressedConv2D.from_codes).parameters) == \
        ["kernel_size", "cin", "cout", "pad", "labels", "centers", "bias", "bias_codes", "activation", "zero_symbol"]
