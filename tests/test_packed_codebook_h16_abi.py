"""CPU checks of the C ABI of the 2- / 4-bit packed codebook layer on bf16 / fp16 activations (include/nnc_cbpk_h16.h, nnc_cbpk_h16 /
nnc_cbpk_dx_h16 / nnc_cbpk_dc_h16): the header against the bound signatures, the plan equalities over CU counts
(forward: nnc_cbpk_grouped_plan with one group; backward, m <= 16: the float32 packed plans field for field; m > 16: the byte form's
half plans at label_bytes = 1 in every shared field), the regimes the case list of tests/helpers/packed_h16_ref.py hits, every
argument error (returned before any HIP call, so none of this needs a device) and the Python errors that need none."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from neural_network_compression_amd import compressed, ops
from neural_network_compression_amd.common import trainer
from tests.helpers import cbgrad_ref, h16_ref
from tests.helpers import packed_h16_ref as pref
from tests.helpers import packed_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NNC_EINVAL, NNC_ENOSPACE = -1, -2
P = 0x1000   # a fake, never dereferenced, 256-byte aligned address
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
CUS = (1, 80, 256, 1024)
NAMES = {f"nnc_cbpk{d}_h16{s}" for d in ("", "_dx", "_dc") for s in ("_workspace_bytes", "_plan", "")}


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_symbols_header_and_signatures_agree(lib):
    """every prototype of include/nnc_cbpk_h16.h is exported and bound with the arguments it declares, from a table of its own; nnc.h
    includes the header and build.py compiles the unit"""
    text = open(os.path.join(ROOT, "include", "nnc_cbpk_h16.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(int64_t|int)\s+(nnc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    assert {p[1] for p in protos} == set(nat.PACKED_H16_SIGNATURES) == NAMES and len(protos) == 9
    assert not set(nat.PACKED_H16_SIGNATURES) & set(nat.SIGNATURES)
    raw = ctypes.CDLL(nat.lib_path())
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64}
    for ret, name, args in protos:
        res, argtypes = nat.PACKED_H16_SIGNATURES[name]
        assert hasattr(raw, name) and res is ctype[ret]
        decl = [a.strip() for a in args.split(",")]
        assert len(decl) == len(argtypes), name
        for d, a in zip(decl, argtypes):
            if "*" in d:
                assert a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)), (name, d)
            else:
                assert a is ctype[d.split()[0]], (name, d)
    assert '#include "nnc_cbpk_h16.h"' in open(os.path.join(ROOT, "include", "nnc.h")).read()
    assert os.path.join(nbuild.CSRC, "nnc_cbpk_h16.hip") in nbuild.SOURCES
    assert nat.CBPKGRAD_H16_PLAN_LEN == len(nat.CBPKDX_H16_PLAN_FIELDS) == len(nat.CBPKDC_H16_PLAN_FIELDS) == 13
    assert nat.CBPK_H16_PLAN_LEN == len(nat.CBPK_H16_PLAN_FIELDS) == 15
    assert nat.CBPKDX_H16_PLAN_FIELDS[:-1] == nat.CBPKDX_PLAN_FIELDS and nat.CBPKDC_H16_PLAN_FIELDS[:-1] == nat.CBPKDC_PLAN_FIELDS
    assert nat.CBPK_H16_PLAN_FIELDS[:-1] == nat.CBPK_PLAN_FIELDS


SHAPES = [(1, 37, 208), (7, 1000, 3000), (16, 4096, 4096), (16, 5000, 5000), (17, 100, 100), (40, 100, 330), (130, 33, 129), (200, 1, 513),
          (512, 784, 300), (512, 4096, 4096), (4096, 4096, 4096), (4096, 5000, 5000), (100000, 70, 129), (64, 130, 100000)]
DX_SHARED = ("path", "splits", "cps", "col_tiles", "row_tiles", "workspace", "dtype")
DC_SHARED = ("path", "splits", "rps", "col_tiles", "row_tiles", "terms_log2", "workspace", "dtype")


@pytest.mark.parametrize("dtype", h16_ref.DTYPES)
@pytest.mark.parametrize("bits,k", [(2, 1), (2, 4), (4, 5), (4, 16)])
@pytest.mark.parametrize("m,kdim,ncols", SHAPES)
def test_backward_plans_equal_the_plans_they_follow(lib, m, kdim, ncols, bits, k, dtype):
    """m <= 16: nnc_cbpk_dx_plan / nnc_cbpk_dc_plan field for field.  m > 16: every field shared with nnc_cbmm_dx_h16_plan /
    nnc_cbmm_dc_h16_plan at label_bytes = 1 (tiles, splits, per-split extent, TERMS_LOG2, workspace), PATH = NNC_CBMM_MFMA, the table
    and the bins the packed form's.  At 1, 80, 256 and 1024 CUs; the splits depend on the shape alone and never shrink with more."""
    t = TDT[dtype]
    dxs = [ops.cbpk_dx_h16_plan(t, m, kdim, ncols, bits, k, cus) for cus in CUS]
    dcs = [ops.cbpk_dc_h16_plan(t, m, kdim, ncols, bits, k, cus) for cus in CUS]
    for cus, dx, dc in zip(CUS, dxs, dcs):
        assert dx["dtype"] == dc["dtype"] == h16_ref.DT_CODE[dtype]
        if m <= 16:
            a, b = ops.cbpk_dx_plan(m, kdim, ncols, bits, k, cus), ops.cbpk_dc_plan(m, kdim, ncols, bits, k, cus)
            assert all(dx[f] == v for f, v in a.items()) and all(dc[f] == v for f, v in b.items())
            assert dx["path"] == dc["path"] == h16_ref.PATH_STREAM
        else:
            a, b = ops.cbmm_dx_h16_plan(t, m, kdim, ncols, 1, k, cus), ops.cbmm_dc_h16_plan(t, m, kdim, ncols, 1, k, cus)
            assert all(dx[f] == a[f] for f in DX_SHARED) and all(dc[f] == b[f] for f in DC_SHARED)
            assert dx["path"] == dc["path"] == h16_ref.PATH_MFMA
            assert dx["vb"] == dx["mt"] == dx["cols"] == dc["vb"] == dc["mt"] == dc["cols"] == 0
            assert dx["cps"] % 32 == 0 and dc["rps"] % 32 == 0
            assert (dx["entries"], dx["copies"], dc["copies"]) == (1 << bits, 32, 64)
            images = 2 * 128 * 40 * 2
            assert dx["lds"] == (((32 + 1) << bits) + 3) // 4 * 4 * 4 + images and dc["lds"] == images + k * 64 * 8
    assert len({(p["splits"], p["cps"], p["workspace"], p["path"]) for p in dxs}) == 1
    assert len({(p["splits"], p["rps"], p["workspace"], p["path"], p["terms_log2"], p["copies"]) for p in dcs}) == 1
    assert dxs[0]["workspace"] == lib.nnc_cbpk_dx_h16_workspace_bytes(m, kdim, ncols, bits)
    assert dcs[0]["workspace"] == lib.nnc_cbpk_dc_h16_workspace_bytes(m, kdim, ncols, bits, k) == 64 + 8 * k
    # the splits of dc and T are the byte form's half plan's at every m: S and the images are that call's
    b = ops.cbmm_dc_h16_plan(t, m, kdim, ncols, 1, k, 256)
    assert all(dcs[0][f] == b[f] for f in ("splits", "rps", "terms_log2"))


@pytest.mark.parametrize("dtype", h16_ref.DTYPES)
@pytest.mark.parametrize("bits,k", [(2, 3), (4, 16)])
@pytest.mark.parametrize("m,kdim,ncols", SHAPES + [(3, 0, 9), (0, 5, 9), (5, 5, 0)])
def test_forward_plan_is_the_grouped_plan_with_one_group(lib, m, kdim, ncols, bits, k, dtype):
    group_rows = max(32, 32 * -(-kdim // 32))
    for cus in CUS:
        p = ops.cbpk_h16_plan(TDT[dtype], m, kdim, ncols, bits, k, cus)
        g = ops.cbpk_grouped_plan(TDT[dtype], m, kdim, ncols, bits, k, group_rows, cus)
        assert all(p[f] == g[f] for f in p) and g["groups"] <= 1
        if min(m, kdim, ncols) > 0:
            assert p["path"] == (h16_ref.PATH_MFMA if m > 16 else h16_ref.PATH_STREAM)
    assert ops.cbpk_h16_plan(TDT[dtype], m, kdim, ncols, bits, k, 256)["workspace"] == lib.nnc_cbpk_h16_workspace_bytes(m, kdim, ncols, bits)
    assert lib.nnc_cbpk_h16_workspace_bytes(m, kdim, ncols, bits) == lib.nnc_cbpk_grouped_workspace_bytes(1, m, kdim, ncols, bits)


@pytest.mark.parametrize("cus", [80, 256, 304])
def test_cases_cover_every_regime(lib, cus):
    dxs, dcs = set(), set()
    for c in pref.CASES:
        _, m, kdim, ncols, bits, k, _, _ = c[0]
        for dtype in h16_ref.DTYPES:
            dxs.add(pref.regime_of(c, ops.cbpk_dx_h16_plan(TDT[dtype], m, kdim, ncols, bits, k, cus), dtype))
            dcs.add(pref.regime_of(c, ops.cbpk_dc_h16_plan(TDT[dtype], m, kdim, ncols, bits, k, cus), dtype))
    assert pref.required_regimes("dx") <= dxs, pref.required_regimes("dx") - dxs
    assert pref.required_regimes("dc") <= dcs, pref.required_regimes("dc") - dcs
    arms = {pref.xvec_arms(c) for c in pref.FULL if c[0][1] > 16}
    assert {a[0] for a in arms} == {True, False} and {a[1] for a in arms} == {True, False}
    assert any(c[0][7] for c in pref.FULL) and {c[0][5] for c in pref.FULL} >= {1, 3, 4, 5, 16}
    assert len(pref.CASES) == 16 and len(pref.MFMA_FORWARD) == 7
    # the forward list: the stream plans split and direct at both widths (packed_ref's cases), the MFMA tile direct and split
    fw = set()
    for c in packed_ref.PACKED_REGIME_CASES:
        p = ops.cbpk_h16_plan(torch.bfloat16, c["m"], c["kdim"], c["ncols"], c["bits"], c["k"], cus)
        fw.add((p["path"], c["bits"], p["splits"] > 1))
    assert {(h16_ref.PATH_STREAM, b, s) for b in (2, 4) for s in (False, True)} <= fw
    assert {(h16_ref.PATH_MFMA, b, s) for b in (2, 4) for s in (False, True)} <= fw


def fw_call(lib, x=P, dt=1, m=4, kdim=8, packed=P, packed_bytes=None, bits=4, ncols=16, centers=P, k=16, y=P, y_dt=0, ws=P, ws_bytes=None):
    if packed_bytes is None:
        packed_bytes = lib.nnc_cbpk_pack_bytes(kdim, ncols, bits) if min(kdim, ncols) >= 0 and bits in (2, 4) else 1 << 20
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbpk_h16_workspace_bytes(m, kdim, ncols, bits) if min(m, kdim, ncols) >= 0 else 0
    return lib.nnc_cbpk_h16(x, dt, m, kdim, packed, packed_bytes, bits, ncols, centers, k, None, 0, y, y_dt, ws, ws_bytes, None)


def dx_call(lib, g=P, dt=1, m=4, kdim=8, packed=P, packed_bytes=None, bits=4, ncols=16, centers=P, k=16, dx=P, dx_dt=0, ws=P, ws_bytes=None):
    if packed_bytes is None:
        packed_bytes = lib.nnc_cbpk_pack_bytes(kdim, ncols, bits) if min(kdim, ncols) >= 0 and bits in (2, 4) else 1 << 20
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbpk_dx_h16_workspace_bytes(m, kdim, ncols, bits) if min(m, kdim, ncols) >= 0 else 0
    return lib.nnc_cbpk_dx_h16(g, dt, m, kdim, packed, packed_bytes, bits, ncols, centers, k, dx, dx_dt, ws, ws_bytes, None)


def dc_call(lib, x=P, g=P, dt=2, m=4, kdim=8, packed=P, packed_bytes=None, bits=4, ncols=16, k=16, dc=P, f64=1, ws=P, ws_bytes=None):
    if packed_bytes is None:
        packed_bytes = lib.nnc_cbpk_pack_bytes(kdim, ncols, bits) if min(kdim, ncols) >= 0 and bits in (2, 4) else 1 << 20
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbpk_dc_h16_workspace_bytes(m, kdim, ncols, bits, k) if min(m, kdim, ncols) >= 0 and 1 <= k <= 16 else 0
    return lib.nnc_cbpk_dc_h16(x, g, dt, m, kdim, packed, packed_bytes, bits, ncols, k, dc, f64, ws, ws_bytes, None)


# (arguments, a piece of the message): section 22's errors (the dtypes, the addresses) and section 14's / 15's (the sizes, the form)
BAD = [(dict(dt=0), "x_dtype must be NNC_DT_BF16 or NNC_DT_F16"), (dict(dt=3), "x_dtype"), (dict(dt=-1), "x_dtype"),
       (dict(m=-1), "negative size"), (dict(kdim=-1), "negative size"), (dict(ncols=-1), "negative size"),
       (dict(bits=3), "bits must be 2 or 4"), (dict(bits=8), "bits must be 2 or 4"), (dict(bits=0), "bits must be 2 or 4"),
       (dict(k=0), "k outside 1..2^bits"), (dict(k=17), "k outside 1..2^bits"), (dict(k=5, bits=2), "k outside 1..2^bits"),
       (dict(m=1 << 41), "size too large"), (dict(kdim=1 << 41), "size too large"), (dict(ncols=1 << 41, kdim=1), "size too large"),
       (dict(packed_bytes=10), "packed_bytes is not nnc_cbpk_pack_bytes"), (dict(packed=None), "packed is NULL"),
       (dict(packed=P + 8), "packed must be 16-byte aligned"), (dict(ws_bytes=-1), "negative workspace size")]


@pytest.mark.parametrize("kw,msg", BAD + [(dict(centers=None), "centers is NULL"), (dict(y=None), "y is NULL"), (dict(x=None), "x is NULL"),
                                          (dict(y_dt=2), "y_dtype must be NNC_DT_F32 or x_dtype"), (dict(y_dt=3), "y_dtype"),
                                          (dict(x=P + 1), "not aligned to its element size"), (dict(y=P + 2), "not aligned to its element size"),
                                          (dict(y=P + 1, y_dt=1), "not aligned to its element size"),
                                          (dict(m=4, kdim=1100, ncols=16, ws=None), "workspace is NULL")])
def test_forward_bad_arguments_are_einval_without_a_device(lib, kw, msg):
    assert fw_call(lib, **kw) == NNC_EINVAL
    err = lib.nnc_last_error().decode()
    assert err.startswith("nnc_cbpk_h16: ") and msg in err, err


@pytest.mark.parametrize("kw,msg", BAD + [(dict(m=1 << 30, kdim=1 << 30, ncols=1), "size too large"),
                                          (dict(centers=None), "centers is NULL"), (dict(dx=None), "dx is NULL"), (dict(g=None), "g is NULL"),
                                          (dict(dx_dt=2), "dx_dtype must be NNC_DT_F32 or x_dtype"), (dict(dx_dt=3), "dx_dtype"),
                                          (dict(g=P + 1), "not aligned to its element size"), (dict(dx=P + 2), "not aligned to its element size"),
                                          (dict(dx=P + 1, dx_dt=1), "not aligned to its element size"),
                                          (dict(m=40, ncols=330, ws=None), "workspace is NULL"), (dict(m=40, ncols=330, ws=P + 2), "workspace must be 4-byte aligned")])
def test_dx_bad_arguments_are_einval_without_a_device(lib, kw, msg):
    assert dx_call(lib, **kw) == NNC_EINVAL
    err = lib.nnc_last_error().decode()
    assert err.startswith("nnc_cbpk_dx_h16: ") and msg in err, err


@pytest.mark.parametrize("kw,msg", BAD + [(dict(m=1 << 30, kdim=1 << 30, ncols=1), "size too large"),
                                          (dict(x=None), "x or g is NULL"), (dict(g=None), "x or g is NULL"), (dict(x=P + 1), "not aligned to its element size"),
                                          (dict(g=P + 1), "not aligned to its element size"), (dict(dc=None), "dc is NULL"),
                                          (dict(ws=None), "workspace is NULL"), (dict(ws=P + 4), "workspace not 8-byte aligned")])
def test_dc_bad_arguments_are_einval_without_a_device(lib, kw, msg):
    assert dc_call(lib, **kw) == NNC_EINVAL
    err = lib.nnc_last_error().decode()
    assert err.startswith("nnc_cbpk_dc_h16: ") and msg in err, err


def test_short_workspace_is_enospace_without_a_device(lib):
    need = lib.nnc_cbpk_dx_h16_workspace_bytes(40, 100, 330, 2)
    assert need == ops.cbmm_dx_h16_plan(torch.bfloat16, 40, 100, 330, 1, 4, 256)["workspace"] > 0
    assert dx_call(lib, m=40, kdim=100, ncols=330, bits=2, k=4, ws_bytes=need - 1) == NNC_ENOSPACE
    assert "workspace smaller than nnc_cbpk_dx_h16_workspace_bytes()" in lib.nnc_last_error().decode()
    need = lib.nnc_cbpk_dx_h16_workspace_bytes(5, 129, 700, 2)
    assert need == lib.nnc_cbpk_dx_workspace_bytes(5, 129, 700, 2) > 0                     # m <= 16: the float32 packed plan's
    assert dx_call(lib, m=5, kdim=129, ncols=700, bits=2, k=3, ws_bytes=need - 1) == NNC_ENOSPACE
    need = lib.nnc_cbpk_dc_h16_workspace_bytes(40, 100, 330, 4, 16)
    assert need == 64 + 8 * 16
    assert dc_call(lib, m=40, kdim=100, ncols=330, ws_bytes=need - 1) == NNC_ENOSPACE
    assert "workspace smaller than nnc_cbpk_dc_h16_workspace_bytes()" in lib.nnc_last_error().decode()
    need = lib.nnc_cbpk_h16_workspace_bytes(4, 1100, 16, 4)
    assert need > 0 and fw_call(lib, m=4, kdim=1100, ncols=16, ws_bytes=need - 1) == NNC_ENOSPACE
    assert lib.nnc_last_error().decode().startswith("nnc_cbpk_h16: ")
    assert lib.nnc_cbpk_dx_h16_workspace_bytes(-1, 1, 1, 4) == 0 and lib.nnc_cbpk_dc_h16_workspace_bytes(1, 1, 1, 3, 1) == 0
    assert lib.nnc_cbpk_h16_workspace_bytes(1, 1, 1, 3) == 0
    # the empty shapes need nothing and are accepted without buffers
    assert fw_call(lib, m=0, x=None, y=None, ws=None) == 0 and dx_call(lib, m=0, g=None, dx=None, ws=None) == 0


@pytest.mark.parametrize("plan,n", [("nnc_cbpk_h16_plan", 15), ("nnc_cbpk_dx_h16_plan", 13), ("nnc_cbpk_dc_h16_plan", 13)])
def test_plan_argument_errors_and_empty_shapes(lib, plan, n):
    fn = getattr(lib, plan)
    out = (ctypes.c_int64 * n)()
    for args, msg in (((1, 4, 8, 16, 4, 16, 0, out), "cus < 1"), ((1, 4, 8, 16, 4, 16, 256, None), "out is NULL"),
                      ((0, 4, 8, 16, 4, 16, 256, out), "x_dtype must be NNC_DT_BF16 or NNC_DT_F16"),        # float32 is not a dtype of these entry points
                      ((1, 4, 8, 16, 2, 5, 256, out), "k outside 1..2^bits"), ((1, 4, 8, 16, 3, 2, 256, out), "bits must be 2 or 4"),
                      ((2, -1, 8, 16, 4, 16, 256, out), "negative size")):
        assert fn(*args) == NNC_EINVAL
        err = lib.nnc_last_error().decode()
        assert err.startswith(plan + ": ") and msg in err, err
    if plan == "nnc_cbpk_h16_plan":
        return
    # empty shapes follow section 15: m = 0 or kdim = 0: dx is empty; ncols = 0: dx = 0; any empty dimension: dc = 0
    for m, kdim, ncols in ((0, 50, 60), (4, 0, 60), (4, 50, 0), (20, 50, 0), (0, 0, 0)):
        assert fn(2, m, kdim, ncols, 4, 8, 256, out) == 0
        f32 = (ops.cbpk_dc_plan if plan.endswith("dc_h16_plan") else ops.cbpk_dx_plan)(m, kdim, ncols, 4, 8, 256)
        assert list(out)[:12] == list(f32.values()) and out[12] == 2
        assert out[0] == (cbgrad_ref.PATH_NONE if "dx" in plan and not (m and kdim) else cbgrad_ref.PATH_ZERO) and out[11] == 0


def test_python_errors_that_need_no_device():
    for plan in (ops.cbpk_h16_plan, ops.cbpk_dx_h16_plan, ops.cbpk_dc_h16_plan):
        with pytest.raises(TypeError):
            plan(torch.float32, 4, 8, 16, 4, 16, 256)
    g = torch.zeros(3, 16, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="CUDA"):                                     # a half tensor is still refused off the device
        ops.packed_codebook_matmul(g, None, torch.zeros(4))
    with pytest.raises(TypeError, match="CUDA"):
        ops.packed_codebook_matmul_dx(g, None, torch.zeros(4))
    with pytest.raises(TypeError, match="one dtype"):
        ops.packed_codebook_centroid_grad(torch.zeros(3, 8, dtype=torch.float16), g, None)
    with pytest.raises(TypeError, match="one dtype"):
        ops.packed_codebook_centroid_grad(torch.zeros(3, 8), g, None)
    src = inspect.getsource(ops._require_f32_x)
    assert "ops.packed_codebook_linear" in src and "ops.sparse_codebook_linear" in src and "ops.codebook_linear" in src
    for name in ("packed_codebook_matmul", "packed_codebook_matmul_dx"):
        assert inspect.signature(getattr(ops, name)).parameters["out_dtype"].default is None


class _NoLayers(torch.nn.Module):
    """a network without layers: the valid keyword combinations build it"""

    def get_config(self):
        return {}


def test_packed_half_inputs_keyword_errors_need_no_device():
    net = _NoLayers()
    builders = (compressed.compress_network, compressed.compress_network_trainable)
    for build in builders:
        assert inspect.signature(build).parameters["packed_half_inputs"].default is False
        for kw in (dict(), dict(packed=False), dict(sparse=True), dict(sparse="auto")):                 # it needs packed
            with pytest.raises(ValueError, match="packed_half_inputs"):
                build(net, {}, packed_half_inputs=True, **kw)
        for kw in (dict(sparse="auto", packed="auto"), dict(sparse="auto", packed=True), dict(sparse=True, packed="auto")):
            with pytest.raises(ValueError, match="sparse_half_inputs"):                                  # with sparse: both keywords, named
                build(net, {}, packed_half_inputs=True, **kw)
            build(net, {}, packed_half_inputs=True, sparse_half_inputs=True, **kw)
        for packed in (True, "auto"):
            build(net, {}, packed=packed, packed_half_inputs=True)
    with pytest.raises(ValueError, match="compress_network_trainable"):                                  # it needs trainable=False here
        compressed.compress_network(net, {}, trainable=True, packed=True, packed_half_inputs=True)
    with pytest.raises(ValueError, match="trainable=False"):
        compressed._check_packed_half_inputs(True, False, True, False, trainable=True)
    with pytest.raises(ValueError, match="packed_half_inputs"):
        compressed.load_network("unused", net, device="cpu", packed_half_inputs=True)
    with pytest.raises(ValueError, match="sparse_half_inputs"):
        compressed.load_network("unused", net, device="cpu", sparse="auto", packed="auto", packed_half_inputs=True)
    assert inspect.signature(compressed.load_network).parameters["packed_half_inputs"].default is False
    assert inspect.signature(trainer.Trainer.compressed_network).parameters["packed_half_inputs"].default is False
    assert inspect.signature(trainer.Trainer.fine_tune_compressed).parameters["packed_half_inputs"].default is False
    # pinned: what raised without the new keyword still raises the same exception type
    for kw in (dict(packed=True), dict(packed="auto")):
        with pytest.raises(ValueError, match="half_inputs"):
            compressed.compress_network_trainable(net, {}, half_inputs=True, **kw)
    for kw in (dict(sparse=True, packed=True), dict(sparse="auto", packed="auto")):
        with pytest.raises(ValueError, match="sparse_half_inputs"):
            compressed.compress_network_trainable(net, {}, sparse_half_inputs=True, **kw)


def test_fine_tune_compressed_keyword_errors_need_no_device():
    """packed_half_inputs=True without activation_dtype or with packed=False; activation_dtype with packed and without the new keyword
    (the pinned ValueError and its text); sparse without sparse_half_inputs: ValueError, before anything is trained"""
    class Bare(trainer.Trainer):   # the abstract parts are never reached: the keyword checks come first
        model_name = "bare"

        def _get_error(self, *a):
            raise AssertionError

        def _layers_to_prune_with_threshold(self, *a):
            raise AssertionError

    t = Bare.__new__(Bare)
    t.quantized_models_by_layer = {object(): [None, None]}
    t.neural_network = torch.nn.Module()
    for kw in (dict(packed=True, packed_half_inputs=True), dict(packed=False, packed_half_inputs=True, activation_dtype=torch.bfloat16),
               dict(packed_half_inputs=True, activation_dtype=torch.float16)):
        with pytest.raises(ValueError, match="packed_half_inputs"):
            t.fine_tune_compressed(None, None, epochs=1, **kw)
    for kw in (dict(packed=True), dict(packed="auto"), dict(sparse="auto", packed="auto")):
        with pytest.raises(ValueError, match="the packed forms do not train on bfloat16 / float16 inputs"):
            t.fine_tune_compressed(None, None, epochs=1, activation_dtype=torch.bfloat16, **kw)
    with pytest.raises(ValueError, match="sparse_half_inputs"):
        t.fine_tune_compressed(None, None, epochs=1, activation_dtype=torch.bfloat16, sparse="auto", packed="auto", packed_half_inputs=True)
    with pytest.raises(ValueError, match="sparse_half_inputs"):                                          # pinned
        t.fine_tune_compressed(None, None, epochs=1, activation_dtype=torch.float16, sparse=True, packed=True, sparse_half_inputs=True)
    with pytest.raises(ValueError, match="activation_dtype"):
        t.fine_tune_compressed(None, None, epochs=1, activation_dtype=torch.float64, packed=True, packed_half_inputs=True)


def test_layer_signatures():
    """half_inputs is the last keyword, default False, of the constructors and of from_dense / from_conv / from_codes of the four packed
    layers; everything in front of it is what it was"""
    for cls in (compressed.PackedCompressedDense, compressed.PackedCompressedConv2D, compressed.TrainablePackedCompressedDense,
                compressed.TrainablePackedCompressedConv2D):
        fns = [cls.__init__, cls.from_codes, getattr(cls, "from_dense", None) or cls.from_conv]
        for fn in fns:
            params = list(inspect.signature(fn).parameters.values())
            assert params[-1].name == "half_inputs" and params[-1].default is False, fn
            assert params[-2].name in ("activation", "bits"), fn
    assert list(inspect.signature(compressed.TrainablePackedCompressedDense.from_codes).parameters)[:-1] == \
        ["kdim", "ncols", "labels", "centers", "bias", "bias_codes", "activation", "bits"]
    assert list(inspect.signature(compressed.PackedCompressedConv2D.from_codes).parameters)[:-1] == \
        ["kernel_size", "cin", "cout", "pad", "labels", "centers", "bias", "activation", "bits"]
