"""CPU checks of the C ABI of the group-wise bitmap-sparse layer on bf16 / fp16 activations (include/nnc_cbsp_grouped_h16.h,
nnc_cbsp_grouped_h16): the header against the bound signatures, the plan against the two plans it is defined by
(nnc_cbmm_grouped_plan of the same dtype for m > 16, nnc_cbsp_grouped_plan for m <= 16), the regimes and group walks the case list of
tests/helpers/grouped_sparse_h16_ref.py reaches, every argument error with its message (returned before any HIP call, so none of
this needs a device) and the Python errors that need none."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from neural_network_compression_amd import compressed, ops
from tests.helpers import grouped_sparse_h16_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NNC_EINVAL, NNC_ENOSPACE = -1, -2
P = 0x1000   # a fake, never dereferenced address (256-byte aligned)
SYMBOLS = {"nnc_cbsp_grouped_h16", "nnc_cbsp_grouped_h16_plan", "nnc_cbsp_grouped_h16_workspace_bytes"}
SHARED_WITH_BYTE_FORM = {"path", "mt", "copies", "entries", "splits", "rps", "lds", "col_tiles", "row_tiles", "workspace", "dtype", "group_rows", "groups",
                         "max_groups_per_split"}


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_symbols_header_and_signatures_agree(lib):
    """every prototype of include/nnc_cbsp_grouped_h16.h is exported and bound with the argument types it declares; nnc.h includes it;
    build.py compiles the unit and watches the header; the tables of the float32 form are as they were"""
    text = open(os.path.join(ROOT, "include", "nnc_cbsp_grouped_h16.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\b(int64_t|int)\s+(nnc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    assert {p[1] for p in protos} == set(nat.GROUPED_SPARSE_H16_SIGNATURES) == SYMBOLS
    assert not set(nat.GROUPED_SPARSE_H16_SIGNATURES) & (set(nat.SIGNATURES) | set(nat.GROUPED_SPARSE_SIGNATURES) | set(nat.SPARSE_H16_SIGNATURES))
    raw = ctypes.CDLL(nat.lib_path())
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "int32_t": ctypes.c_int32}
    for ret, name, args in protos:
        res, argtypes = nat.GROUPED_SPARSE_H16_SIGNATURES[name]
        assert hasattr(raw, name) and res is ctype[ret]
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is res
        decl = [a.strip() for a in args.split(",")]
        assert len(decl) == len(argtypes), name
        for d, a in zip(decl, argtypes):
            if "*" in d:
                assert a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)), (name, d)
            else:
                assert a is ctype[d.split()[0]], (name, d)
    assert '#include "nnc_cbsp_grouped_h16.h"' in open(os.path.join(ROOT, "include", "nnc.h")).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (NNC_\w+) (\d+)", text)}
    assert defs["NNC_CBSP_GROUPED_H16_PLAN_LEN"] == nat.CBSP_GROUPED_H16_PLAN_LEN == len(nat.CBSP_GROUPED_H16_PLAN_FIELDS) == 15
    assert defs["NNC_CBSP_GROUPED_H16_P_DTYPE"] == nat.CBSP_GROUPED_H16_PLAN_FIELDS.index("dtype") == 14
    assert nat.CBSP_GROUPED_H16_PLAN_FIELDS[:14] == nat.CBSP_GROUPED_PLAN_FIELDS
    assert os.path.join(nbuild.CSRC, "nnc_cbsp_grouped_h16.hip") in nbuild.SOURCES
    assert os.path.join(nbuild.INCLUDE, "nnc_cbsp_grouped_h16.h") in nbuild._headers()
    assert os.path.join(nbuild.CSRC, "nnc_cbsp_grouped.hpp") in nbuild._headers()


@pytest.mark.parametrize("dtype", ref.DTYPES)
@pytest.mark.parametrize("case", ref.CASES, ids=[ref.case_id(c) for c in ref.CASES])
def test_the_plan_is_the_grouped_byte_forms_half_plan_above_16_rows_and_the_grouped_sparse_plan_below(lib, case, dtype):
    m, kdim, ncols, k, gr = (case[n] for n in ("m", "kdim", "ncols", "k", "group_rows"))
    tdt, code = ref.torch_dtype(dtype), ref.DT_CODE[dtype]
    for cus in ref.CU_COUNTS:
        p = ops.cbsp_grouped_h16_plan(tdt, m, kdim, ncols, k, gr, cus)
        assert tuple(p) == nat.CBSP_GROUPED_H16_PLAN_FIELDS and p["dtype"] == code
        if m > 16:
            q = ops.cbmm_grouped_plan(tdt, m, kdim, ncols, k, gr, cus)
            assert set(p) & set(q) == SHARED_WITH_BYTE_FORM
            assert all(p[f] == q[f] for f in SHARED_WITH_BYTE_FORM), (p, q)
            assert p["path"] == ref.PATH_MFMA and p["rps"] % 32 == 0 and p["rowsum"] == nat.CBSP_ROWSUM_NONE and p["lds"] <= 64 * 1024
        else:
            q = ops.cbsp_grouped_plan(m, kdim, ncols, k, gr, cus)
            assert set(q) == set(p) - {"dtype"}
            assert all(p[f] == v for f, v in q.items()), (p, q)
            assert p["path"] == ref.PATH_STREAM and p["rowsum"] == nat.CBSP_ROWSUM_PASS
        assert p["workspace"] <= lib.nnc_cbsp_grouped_h16_workspace_bytes(code, m, kdim, ncols)
    # the query plans for 256 CUs, and more CUs change nothing
    assert ops.cbsp_grouped_h16_plan(tdt, m, kdim, ncols, k, gr, 256)["workspace"] == lib.nnc_cbsp_grouped_h16_workspace_bytes(code, m, kdim, ncols)
    assert ops.cbsp_grouped_h16_plan(tdt, m, kdim, ncols, k, gr, 1024) == ops.cbsp_grouped_h16_plan(tdt, m, kdim, ncols, k, gr, 256)


@pytest.mark.parametrize("m,kdim,ncols,gr", [(1, 4096, 4096, 128), (16, 4096, 4096, 32), (256, 4096, 4096, 128), (4096, 4096, 4096, 32),
                                              (100000, 96, 129, 32), (33, 5000, 5000, 160)])
def test_the_plan_equalities_hold_at_the_measured_shapes(lib, m, kdim, ncols, gr):
    for dtype in ref.DTYPES:
        tdt = ref.torch_dtype(dtype)
        for cus in ref.CU_COUNTS:
            p = ops.cbsp_grouped_h16_plan(tdt, m, kdim, ncols, 16, gr, cus)
            q = ops.cbmm_grouped_plan(tdt, m, kdim, ncols, 16, gr, cus) if m > 16 else ops.cbsp_grouped_plan(m, kdim, ncols, 16, gr, cus)
            assert all(p[f] == q[f] for f in set(p) & set(q)), (p, q)


def test_the_case_list_reaches_every_regime_and_group_walk_at_256_cus(lib):
    hit, feats = set(), set()
    for c in ref.CASES:
        for dtype in ref.DTYPES:
            plan = ops.cbsp_grouped_h16_plan(ref.torch_dtype(dtype), c["m"], c["kdim"], c["ncols"], c["k"], c["group_rows"], 256)
            hit.add(ref.regime_of(plan, dtype))
            feats |= ref.features_of(c, plan)
    assert hit == ref.required_regimes(), sorted(ref.required_regimes() ^ hit)
    assert feats >= ref.required_features(), sorted(ref.required_features() - feats)
    for big in (False, True):
        mine = [c for c in ref.CASES if (c["m"] > 16) == big]
        assert {c["k"] for c in mine} == {3, 16, 256} and {c["bias"] for c in mine} == {True, False}
        assert any(c["off"] % 2 for c in mine) and any(c["x_view"] for c in mine) and any(c["ncols"] % 64 for c in mine)


def call(lib, x=P, dt=1, m=4, kdim=64, packed=P, packed_bytes=None, ncols=16, zs=P, nnz=10, centers=P, k=16, group_rows=32, y=P, y_dt=0, ws=P, ws_bytes=None):
    ok = min(m, kdim, ncols) >= 0
    if packed_bytes is None:
        packed_bytes = lib.nnc_cbsp_pack_bytes(kdim, ncols, 1, max(nnz, 0)) if ok else 0
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbsp_grouped_h16_workspace_bytes(dt, m, kdim, ncols) if ok else 0
    return lib.nnc_cbsp_grouped_h16(x, dt, m, kdim, packed, packed_bytes, ncols, zs, nnz, centers, k, group_rows, None, 0, y, y_dt, ws, ws_bytes, None)


BAD = [(dict(dt=0), "x_dtype must be"), (dict(dt=3), "x_dtype must be"), (dict(dt=-1), "x_dtype must be"),
       (dict(m=-1), "negative size"), (dict(kdim=-1), "negative size"), (dict(ncols=-1), "negative size"),
       (dict(m=1 << 41), "size too large"), (dict(ncols=1 << 32, nnz=0), "size too large"), (dict(kdim=1 << 41, ncols=1, nnz=0), "size too large"),
       (dict(k=0), "k outside 1..256"), (dict(k=-3), "k outside 1..256"), (dict(k=257), "k outside 1..256"), (dict(k=1040), "k outside 1..256"),
       (dict(group_rows=0), "group_rows must be a positive multiple of 32"), (dict(group_rows=-32), "group_rows must be a positive multiple of 32"),
       (dict(group_rows=16), "group_rows must be a positive multiple of 32"), (dict(group_rows=48), "group_rows must be a positive multiple of 32"),
       (dict(group_rows=1 << 41), "size too large"),
       (dict(nnz=-1), "nnz outside"), (dict(nnz=64 * 16 + 1), "nnz outside"), (dict(packed_bytes=100), "packed buffer smaller"),
       (dict(y_dt=2), "y_dtype must be"), (dict(y_dt=3), "y_dtype must be"), (dict(dt=2, y_dt=1), "y_dtype must be"),
       (dict(centers=None), "centers is NULL"), (dict(y=None), "y is NULL"), (dict(x=None), "x, packed or zero_symbols is NULL"),
       (dict(packed=None), "x, packed or zero_symbols is NULL"), (dict(zs=None), "x, packed or zero_symbols is NULL"),
       (dict(x=P + 1), "not aligned"), (dict(y=P + 2), "not aligned"), (dict(y=P + 1, y_dt=1), "not aligned"),
       (dict(packed=P + 128), "256-byte aligned"), (dict(ws_bytes=-1), "negative workspace size"),
       (dict(ws=None), "workspace is NULL"), (dict(ws=P + 2), "workspace must be 4-byte aligned"),
       (dict(m=40, kdim=300, ncols=300, nnz=0, ws=None), "workspace is NULL"), (dict(m=40, kdim=300, ncols=300, nnz=0, ws=P + 2), "workspace must be 4-byte aligned")]


@pytest.mark.parametrize("kw,msg", BAD, ids=[f"{i}-{'-'.join(kw)}" for i, (kw, _) in enumerate(BAD)])
def test_bad_arguments_are_einval_with_their_message_without_a_device(lib, kw, msg):
    assert call(lib, **kw) == NNC_EINVAL
    text = lib.nnc_last_error().decode()
    assert text.startswith("nnc_cbsp_grouped_h16: ") and msg in text, text


def test_short_workspace_is_enospace_and_the_queries(lib):
    need = lib.nnc_cbsp_grouped_h16_workspace_bytes(1, 40, 300, 300)     # m > 16: the byte form's partials, nothing else
    assert need == ops.cbmm_grouped_plan(torch.bfloat16, 40, 300, 300, 16, 32, 256)["workspace"] == 4 * 40 * 300 * 4
    assert need == lib.nnc_cbmm_grouped_workspace_bytes(1, 40, 300, 300)
    assert call(lib, m=40, kdim=300, ncols=300, nnz=0, ws_bytes=need - 1) == NNC_ENOSPACE
    assert "nnc_cbsp_grouped_h16_workspace_bytes" in lib.nnc_last_error().decode()
    need = lib.nnc_cbsp_grouped_h16_workspace_bytes(2, 1, 5000, 300)     # m <= 16: the float32 form's partials, t and the word behind it
    assert need == lib.nnc_cbsp_grouped_workspace_bytes(1, 5000, 300) > 4 * 1 + 4
    assert call(lib, dt=2, m=1, kdim=5000, ncols=300, nnz=0, ws_bytes=need - 1) == NNC_ENOSPACE
    assert call(lib, m=4, ws_bytes=4 * 4 + 3) == NNC_ENOSPACE            # a direct stream call still needs t and the word
    assert lib.nnc_cbsp_grouped_h16_workspace_bytes(1, 17, 64, 16) == 0  # a direct MFMA call needs nothing
    for bad in ((0, 4, 64, 16), (3, 4, 64, 16), (1, -1, 5, 5), (1, 1 << 41, 1, 1), (1, 1, 1, 1 << 32)):
        assert lib.nnc_cbsp_grouped_h16_workspace_bytes(*bad) == 0
    for empty in ((1, 0, 5, 5), (2, 5, 0, 5), (1, 5, 5, 0)):
        assert lib.nnc_cbsp_grouped_h16_workspace_bytes(*empty) == 0


def test_empty_calls_return_before_any_device_work(lib):
    """m = 0 or ncols = 0 is a no-op: NNC_OK with never-dereferenced pointers and no device"""
    assert call(lib, m=0, x=None, y=None, ws=None, ws_bytes=0) == 0
    assert call(lib, ncols=0, nnz=0, x=None, y=None, ws=None, ws_bytes=0) == 0
    assert call(lib, m=0, kdim=0, nnz=0, x=None, packed=None, zs=None, y=None, ws=None, ws_bytes=0) == 0


def test_plan_argument_errors_and_empty_shapes(lib):
    fn = lib.nnc_cbsp_grouped_h16_plan
    out = (ctypes.c_int64 * 15)()
    for args, msg in (((1, 4, 64, 16, 16, 32, 0, out), "cus < 1"), ((1, 4, 64, 16, 16, 32, 256, None), "out is NULL"),
                      ((0, 4, 64, 16, 16, 32, 256, out), "x_dtype must be"), ((1, 4, 64, 16, 300, 32, 256, out), "k outside 1..256"),
                      ((2, -1, 64, 16, 16, 32, 256, out), "negative size"), ((2, 40, 64, 1 << 32, 16, 32, 256, out), "size too large"),
                      ((2, 40, 64, 16, 16, 48, 256, out), "group_rows must be")):
        assert fn(*args) == NNC_EINVAL, args
        text = lib.nnc_last_error().decode()
        assert text.startswith("nnc_cbsp_grouped_h16_plan: ") and msg in text, text
    for m, kdim, ncols, path in ((0, 64, 60, 0), (4, 64, 0, 0), (20, 64, 0, 0), (4, 0, 60, 3), (20, 0, 60, 3)):
        assert fn(2, m, kdim, ncols, 8, 32, 256, out) == 0
        assert list(out) == [path, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 32, -(-kdim // 32), 0, 2]


def test_python_errors_that_need_no_device():
    with pytest.raises(TypeError, match="bfloat16 or torch.float16"):
        ops.cbsp_grouped_h16_plan(torch.float32, 4, 64, 16, 16, 32, 256)
    with pytest.raises(nat.NncError, match="group_rows"):
        ops.cbsp_grouped_h16_plan(torch.bfloat16, 4, 64, 16, 16, 48, 256)
    for dt in (torch.bfloat16, torch.float16):
        # without the keyword a half x is refused as it always was, and the message now names the keyword
        with pytest.raises(TypeError, match="float32 activations.*half_inputs=True"):
            ops.grouped_sparse_codebook_matmul(torch.zeros(3, 64, dtype=dt), None, torch.zeros(2, 4))
        with pytest.raises(TypeError, match="CUDA"):   # with it a half tensor is still refused off the device
            ops.grouped_sparse_codebook_matmul(torch.zeros(3, 64, dtype=dt), None, torch.zeros(2, 4), half_inputs=True)
    with pytest.raises(TypeError, match="CUDA"):
        ops.grouped_sparse_codebook_matmul(torch.zeros(3, 64), None, torch.zeros(2, 4), half_inputs=True)
    params = inspect.signature(ops.grouped_sparse_codebook_matmul).parameters
    assert list(params)[-2:] == ["out_dtype", "half_inputs"] and params["out_dtype"].default is None and params["half_inputs"].default is False
    layer = compressed.GroupedSparseCompressedDense
    for fn in (layer.__init__, layer.from_dense, layer.from_codes, layer.from_grouped, compressed.sparsify_grouped_layers,
               compressed.smallest_grouped_layers):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "half_inputs" and last.default is False, fn
    with pytest.raises(ValueError, match="sparse must be True or 'auto'"):
        compressed.sparsify_grouped_layers(torch.nn.Module(), sparse=False, half_inputs=True)
    for fn in (ops.grouped_sparse_codebook_matmul, layer, compressed.sparsify_grouped_layers, compressed.smallest_grouped_layers):
        assert "float32 activations only" not in fn.__doc__ and "half_inputs" in fn.__doc__
