"""CPU checks of the C ABI of the bitmap-sparse codebook matmul on bf16 / fp16 activations (include/nnc_cbsp_h16.h, nnc_cbsp_h16,
DESIGN.md section 23): the header against the bound signatures, the plan against the two plans it is defined by (nnc_cbmm_h16_plan
for m > 16, nnc_cbsp_plan for m <= 16), the regimes the case list of tests/helpers/sparse_h16_ref.py hits, every argument error
(returned before any HIP call, so none of this needs a device) and the Python errors that need none."""
import ctypes
import os
import re

import pytest
import torch

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from neural_network_compression_amd import compressed, ops
from tests.helpers import h16_ref
from tests.helpers import sparse_h16_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NNC_EINVAL, NNC_ENOSPACE = -1, -2
P = 0x1000   # a fake, never dereferenced address (256-byte aligned)
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
CUS = (1, 80, 256, 1024)
SHAPES = [(1, 37, 208), (7, 1001, 3000), (16, 4096, 4096), (17, 100, 100), (33, 300, 129), (130, 33, 129), (200, 1, 513), (512, 784, 300),
          (4096, 4096, 4096), (4096, 5000, 5000), (100000, 70, 129)]


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_symbols_header_and_signatures_agree(lib):
    """every prototype of include/nnc_cbsp_h16.h is exported and bound with the argument types it declares; nnc.h includes it"""
    text = open(os.path.join(ROOT, "include", "nnc_cbsp_h16.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(int64_t|int)\s+(nnc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    assert {p[1] for p in protos} == set(nat.SPARSE_H16_SIGNATURES) == {"nnc_cbsp_h16", "nnc_cbsp_h16_plan", "nnc_cbsp_h16_workspace_bytes"}
    assert not set(nat.SPARSE_H16_SIGNATURES) & set(nat.SIGNATURES)
    raw = ctypes.CDLL(nat.lib_path())
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64}
    for ret, name, args in protos:
        res, argtypes = nat.SPARSE_H16_SIGNATURES[name]
        assert hasattr(raw, name) and res is ctype[ret]
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is res
        decl = [a.strip() for a in args.split(",")]
        assert len(decl) == len(argtypes), name
        for d, a in zip(decl, argtypes):
            if "*" in d:
                assert a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)), (name, d)
            else:
                assert a is ctype[d.split()[0]], (name, d)
    assert '#include "nnc_cbsp_h16.h"' in open(os.path.join(ROOT, "include", "nnc.h")).read()
    assert nat.CBSP_H16_PLAN_LEN == len(nat.CBSP_H16_PLAN_FIELDS) == 12 and nat.CBSP_H16_PLAN_FIELDS[:11] == nat.CBSP_PLAN_FIELDS
    assert os.path.join(nbuild.CSRC, "nnc_cbsp_h16.hip") in nbuild.SOURCES


@pytest.mark.parametrize("dtype", h16_ref.DTYPES)
@pytest.mark.parametrize("lb,k", [(1, 17), (1, 256), (2, 257), (2, 1040)])
@pytest.mark.parametrize("m,kdim,ncols", SHAPES)
def test_the_plan_is_the_byte_forms_half_plan_above_16_rows_and_the_sparse_stream_plan_below(lib, m, kdim, ncols, lb, k, dtype):
    for cus in CUS:
        p = ops.cbsp_h16_plan(TDT[dtype], m, kdim, ncols, lb, k, cus)
        assert tuple(p) == nat.CBSP_H16_PLAN_FIELDS and p["dtype"] == h16_ref.DT_CODE[dtype]
        if m > 16:
            q = ops.cbmm_h16_plan(TDT[dtype], m, kdim, ncols, lb, k, cus)
            shared = set(p) & set(q)
            assert shared == {"path", "mt", "copies", "entries", "splits", "rps", "lds", "col_tiles", "row_tiles", "workspace", "dtype"}
            assert all(p[f] == q[f] for f in shared), (p, q)
            assert p["path"] == h16_ref.PATH_MFMA and p["rps"] % 32 == 0 and p["rowsum"] == nat.CBSP_ROWSUM_NONE and p["lds"] <= 64 * 1024
        else:
            q = ops.cbsp_plan(m, kdim, ncols, lb, k, cus)
            assert all(p[f] == v for f, v in q.items()), (p, q)
            assert p["path"] == h16_ref.PATH_STREAM and p["rowsum"] == nat.CBSP_ROWSUM_FUSED
        assert p["workspace"] <= lib.nnc_cbsp_h16_workspace_bytes(m, kdim, ncols, lb)
    # the query plans for 256 CUs, and more CUs change nothing
    assert ops.cbsp_h16_plan(TDT[dtype], m, kdim, ncols, lb, k, 256)["workspace"] == lib.nnc_cbsp_h16_workspace_bytes(m, kdim, ncols, lb)
    assert ops.cbsp_h16_plan(TDT[dtype], m, kdim, ncols, lb, k, 1024) == ops.cbsp_h16_plan(TDT[dtype], m, kdim, ncols, lb, k, 256)


@pytest.mark.parametrize("cus", [80, 256])
def test_cases_cover_every_regime(lib, cus):
    hit = set()
    for c in sref.CASES:
        for dtype in h16_ref.DTYPES:
            hit.add(sref.regime_of(c, ops.cbsp_h16_plan(TDT[dtype], c["m"], c["kdim"], c["ncols"], c["lb"], c["k"], cus), dtype))
    assert hit == sref.required_regimes(), sorted(sref.required_regimes() - hit)
    both = lambda f: {(c["m"] > 16, c[f]) for c in sref.CASES}   # noqa: E731
    assert both("cz_zero") == both("x_view") == both("bias") == both("relu") == {(a, b) for a in (False, True) for b in (False, True)}
    assert {(c["m"] > 16, c["density"]) for c in sref.CASES} == {(a, d) for a in (False, True) for d in sref.DENSITIES + (0.0,)}
    assert {(c["lb"], c["k"]) for c in sref.CASES} == {(1, 17), (1, 256), (2, 257), (2, 1040)}
    assert {c["m"] for c in sref.CASES} == set(sref.MS) and {c["kdim"] for c in sref.CASES} == set(sref.KDIMS)
    assert {c["ncols"] for c in sref.CASES} == set(sref.NCOLS)


def call(lib, x=P, dt=1, m=4, kdim=8, packed=P, packed_bytes=None, lb=1, ncols=16, z=0, nnz=5, centers=P, k=16, y=P, y_dt=0, ws=None, ws_bytes=None):
    ok = min(m, kdim, ncols) >= 0 and lb in (1, 2)
    if packed_bytes is None:
        packed_bytes = lib.nnc_cbsp_pack_bytes(kdim, ncols, lb, max(nnz, 0)) if ok else 0
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbsp_h16_workspace_bytes(m, kdim, ncols, lb) if ok else 0
    return lib.nnc_cbsp_h16(x, dt, m, kdim, packed, packed_bytes, lb, ncols, z, nnz, centers, k, None, 0, y, y_dt, ws, ws_bytes, None)


BAD = [(dict(dt=0), "x_dtype must be"), (dict(dt=3), "x_dtype must be"), (dict(dt=-1), "x_dtype must be"),
       (dict(m=-1), "negative size"), (dict(kdim=-1), "negative size"), (dict(ncols=-1), "negative size"),
       (dict(lb=0), "label_bytes must be 1 or 2"), (dict(lb=3), "label_bytes must be 1 or 2"),
       (dict(m=1 << 41), "size too large"), (dict(ncols=1 << 32, nnz=0), "size too large"), (dict(kdim=1 << 41, ncols=1, nnz=0), "size too large"),
       (dict(k=0), "k outside"), (dict(k=-3), "k outside"), (dict(k=1041, lb=2), "k outside"), (dict(k=257, lb=1), "needs 2-byte labels"),
       (dict(z=-1), "zero_symbol outside"), (dict(z=256), "zero_symbol outside"), (dict(z=65536, lb=2), "zero_symbol outside"),
       (dict(nnz=-1), "nnz outside"), (dict(nnz=8 * 16 + 1), "nnz outside"),
       (dict(packed_bytes=0), "packed buffer smaller"), (dict(y_dt=2), "y_dtype must be"), (dict(y_dt=3), "y_dtype must be"),
       (dict(centers=None), "centers is NULL"), (dict(y=None), "y is NULL"), (dict(x=None), "x or packed is NULL"),
       (dict(packed=None), "x or packed is NULL"), (dict(x=P + 1), "not aligned"), (dict(y=P + 2), "not aligned"), (dict(y=P + 1, y_dt=1), "not aligned"),
       (dict(packed=P + 128), "256-byte aligned"), (dict(ws_bytes=-1), "negative workspace size"),
       (dict(m=40, kdim=300, ws=None), "workspace is NULL"), (dict(m=40, kdim=300, ws=P + 2), "workspace must be 4-byte aligned"),
       (dict(m=4, kdim=1100, nnz=0, ws=None), "workspace is NULL")]


@pytest.mark.parametrize("kw,msg", BAD, ids=[f"{i}-{'-'.join(kw)}" for i, (kw, _) in enumerate(BAD)])
def test_bad_arguments_are_einval_with_their_message_without_a_device(lib, kw, msg):
    assert call(lib, **kw) == NNC_EINVAL
    text = lib.nnc_last_error().decode()
    assert text.startswith("nnc_cbsp_h16: ") and msg in text, text


def test_short_workspace_is_enospace_and_the_queries(lib):
    need = lib.nnc_cbsp_h16_workspace_bytes(40, 300, 300, 2)
    assert need == ops.cbmm_h16_plan(torch.bfloat16, 40, 300, 300, 2, 300, 256)["workspace"] == 4 * 40 * 300 * 4
    assert call(lib, m=40, kdim=300, ncols=300, lb=2, k=300, ws=P, ws_bytes=need - 1) == NNC_ENOSPACE
    assert "nnc_cbsp_h16_workspace_bytes" in lib.nnc_last_error().decode()
    need = lib.nnc_cbsp_h16_workspace_bytes(4, 1100, 16, 1)
    assert need == lib.nnc_cbsp_workspace_bytes(4, 1100, 16, 1) > 0
    assert call(lib, m=4, kdim=1100, nnz=0, ws=P, ws_bytes=need - 1) == NNC_ENOSPACE
    for bad in ((-1, 1, 1, 1), (1, 1, 1, 3), (1, 1, 1 << 32, 1), (1 << 41, 1, 1, 1)):
        assert lib.nnc_cbsp_h16_workspace_bytes(*bad) == 0
    for empty in ((0, 5, 5, 1), (5, 0, 5, 1), (5, 5, 0, 2)):
        assert lib.nnc_cbsp_h16_workspace_bytes(*empty) == 0


def test_empty_calls_return_before_any_device_work(lib):
    """m = 0 or ncols = 0 is a no-op: NNC_OK with never-dereferenced pointers and no device"""
    assert call(lib, m=0, nnz=0) == 0
    assert call(lib, ncols=0, nnz=0) == 0
    assert call(lib, m=0, kdim=0, nnz=0, x=None, packed=None, y=None) == 0


def test_plan_argument_errors_and_empty_shapes(lib):
    fn = lib.nnc_cbsp_h16_plan
    out = (ctypes.c_int64 * 12)()
    for args, msg in (((1, 4, 8, 16, 1, 16, 0, out), "cus < 1"), ((1, 4, 8, 16, 1, 16, 256, None), "out is NULL"),
                      ((0, 4, 8, 16, 1, 16, 256, out), "x_dtype must be"), ((1, 4, 8, 16, 1, 257, 256, out), "needs 2-byte labels"),
                      ((2, -1, 8, 16, 1, 16, 256, out), "negative size"), ((2, 40, 8, 1 << 32, 1, 16, 256, out), "size too large")):
        assert fn(*args) == NNC_EINVAL and msg in lib.nnc_last_error().decode(), args
    for m, kdim, ncols, path in ((0, 50, 60, 0), (4, 50, 0, 0), (20, 50, 0, 0), (4, 0, 60, 3), (20, 0, 60, 3)):
        assert fn(2, m, kdim, ncols, 1, 8, 256, out) == 0
        assert list(out) == [path, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2]


def test_python_errors_that_need_no_device():
    with pytest.raises(TypeError, match="bfloat16 or torch.float16"):
        ops.cbsp_h16_plan(torch.float32, 4, 8, 16, 1, 16, 256)
    with pytest.raises(TypeError, match="CUDA"):                                     # a half tensor is still refused off the device
        ops.sparse_codebook_matmul(torch.zeros(3, 16, dtype=torch.bfloat16), None, torch.zeros(4))
    net = torch.nn.Module()
    for kw in (dict(), dict(sparse=False), dict(sparse=True, trainable=True), dict(sparse="auto", trainable=True), dict(trainable=True)):
        with pytest.raises(ValueError, match="sparse_half_inputs"):
            compressed.compress_network(net, {}, sparse_half_inputs=True, **kw)
    with pytest.raises(ValueError, match="sparse_half_inputs"):
        compressed.load_network("no such file", net, sparse_half_inputs=True)
    import inspect

    from neural_network_compression_amd.common import trainer

    for fn in (compressed.compress_network, compressed.load_network, trainer.Trainer.compressed_network):
        assert inspect.signature(fn).parameters["sparse_half_inputs"].default is False
    for fn in (compressed.SparseCompressedDense.__init__, compressed.SparseCompressedDense.from_dense, compressed.SparseCompressedDense.from_codes,
               compressed.SparseCompressedConv2D.__init__, compressed.SparseCompressedConv2D.from_conv, compressed.SparseCompressedConv2D.from_codes):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == "half_inputs" and params[-1].default is False, fn
    assert "half_inputs" not in inspect.signature(compressed.TrainableSparseCompressedDense.from_codes).parameters   # out of scope: they keep refusing
    assert inspect.signature(ops.sparse_codebook_matmul).parameters["out_dtype"].default is None
