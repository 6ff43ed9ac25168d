"""CPU checks of the C ABI of the group-wise codebook backward pass on bf16 / fp16 activations (include/nnc_cbgrad_grouped_h16.h,
nnc_cbmm_grouped_dx_h16 / _dc_h16 and nnc_cbpk_grouped_dx_h16 / _dc_h16): the header against the bound
signatures, the plans against the ungrouped half plans and the float32 grouped plans over CU counts, the group fields against a
NumPy restatement, the regimes the case lists of tests/helpers/grouped_h16_grad_ref.py hit, every argument error (returned before
any HIP call, so none of this needs a device) and the Python errors that need none."""
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
from tests.helpers import grouped_grad_ref as gref
from tests.helpers import grouped_h16_grad_ref as ref
from tests.helpers.h16_ref import DT_CODE, DTYPES, PATH_MFMA, PATH_STREAM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NNC_EINVAL, NNC_ENOSPACE = -1, -2
P = 0x1000   # a fake, never dereferenced, 16-byte aligned address
TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
TAIL = ("group_rows", "groups", "rows_per_group", "max_groups_per_workgroup", "held")


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def test_symbols_header_and_signatures_agree(lib):
    """every prototype of include/nnc_cbgrad_grouped_h16.h is exported and bound with the arguments it declares, from a table of its own
    that load() requires; nnc.h includes the header once; the units are in build.SOURCES"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nnc_cbgrad_grouped_h16.h")).read(), flags=re.S)
    protos = re.findall(r"\b(int64_t|int)\s+(nnc_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)
    assert {p[1] for p in protos} == set(nat.GROUPED_H16_GRAD_SIGNATURES) and len(protos) == 12
    assert not set(nat.GROUPED_H16_GRAD_SIGNATURES) & set(nat.SIGNATURES)
    raw = ctypes.CDLL(nat.lib_path())
    ctype = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint64_t": ctypes.c_uint64}
    for ret, name, args in protos:
        res, argtypes = nat.GROUPED_H16_GRAD_SIGNATURES[name]
        assert hasattr(raw, name) and res is ctype[ret]
        assert getattr(lib, name).argtypes == argtypes and getattr(lib, name).restype is res
        decl = [a.strip() for a in args.split(",")]
        assert len(decl) == len(argtypes), name
        for d, a in zip(decl, argtypes):
            if "*" in d:
                assert a in (ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)), (name, d)
            else:
                assert a is ctype[d.split()[0]], (name, d)
    assert open(os.path.join(ROOT, "include", "nnc.h")).read().count('#include "nnc_cbgrad_grouped_h16.h"') == 1
    assert "GROUPED_H16_GRAD_SIGNATURES" in inspect.getsource(nat.load)
    for unit in ("nnc_cbgrad_grouped_h16.hip", "nnc_cbpkgrad_grouped_h16.hip"):
        assert os.path.join(nbuild.CSRC, unit) in nbuild.SOURCES
    defs = {k: int(v) for k, v in re.findall(r"#define (NNC_\w+) (\d+)", text)}
    assert defs["NNC_CBGRAD_GROUPED_H16_PLAN_LEN"] == nat.CBGRAD_GROUPED_H16_PLAN_LEN == 18
    for fields, head in ((nat.CBDX_GROUPED_H16_PLAN_FIELDS, nat.CBDX_H16_PLAN_FIELDS), (nat.CBDC_GROUPED_H16_PLAN_FIELDS, nat.CBDC_H16_PLAN_FIELDS),
                         (nat.CBPKDX_GROUPED_H16_PLAN_FIELDS, nat.CBPKDX_H16_PLAN_FIELDS), (nat.CBPKDC_GROUPED_H16_PLAN_FIELDS, nat.CBPKDC_H16_PLAN_FIELDS)):
        assert len(fields) == 18 and fields[:13] == head and fields[13:] == TAIL
        for name in TAIL:
            assert defs["NNC_CBGRAD_GROUPED_H16_P_" + name.upper()] == fields.index(name)


def _group_fields(path, plan, kdim, gr):
    """The five group fields restated: the groups, the rows of a stream workgroup, the most groups a workgroup's rows lie in (a
    128-row tile on the MFMA path) and the tables / sets a tile holds."""
    stream = path == PATH_STREAM
    per = plan["rows_per_group"] if stream else 128
    most = gref.max_groups(None, per, kdim, gr) if path in (PATH_STREAM, PATH_MFMA) and kdim > 0 else 0
    return dict(group_rows=gr, groups=-(-kdim // gr) if kdim > 0 else 0, max_groups_per_workgroup=most)


SHAPES = [(1, 300, 50), (5, 200, 130), (16, 300, 130), (16, 200, 300), (17, 300, 130), (64, 300, 128), (130, 200, 50), (512, 4096, 4096), (4096, 784, 300),
          (0, 50, 60), (4, 0, 60), (20, 0, 60), (4, 50, 0), (20, 50, 0)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("gr", [32, 96, 128, 4096])
@pytest.mark.parametrize("m,kdim,ncols", SHAPES)
def test_byte_plans_are_the_ungrouped_half_plans_plus_the_group_fields(lib, m, kdim, ncols, gr, dtype):
    dt, k = TDT[dtype], 16
    G = max(1, -(-kdim // gr))
    for cus in ref.CU_COUNTS:
        dx, dc = ops.cbmm_grouped_dx_h16_plan(dt, m, kdim, ncols, k, gr, cus), ops.cbmm_grouped_dc_h16_plan(dt, m, kdim, ncols, k, gr, cus)
        udx, udc = ops.cbmm_dx_h16_plan(dt, m, kdim, ncols, 1, k, cus), ops.cbmm_dc_h16_plan(dt, m, kdim, ncols, 1, k, cus)
        assert {f: dx[f] for f in nat.CBDX_H16_PLAN_FIELDS} == udx                                   # every shared field, LDS included
        assert {f: dc[f] for f in nat.CBDC_H16_PLAN_FIELDS if f != "workspace"} == {f: v for f, v in udc.items() if f != "workspace"}   # TERMS_LOG2 included
        empty = m == 0 or kdim == 0 or ncols == 0
        assert dc["workspace"] == (0 if empty else 64 + 8 * G * k) == lib.nnc_cbmm_grouped_dc_h16_workspace_bytes(m, kdim, ncols, k, gr)
        assert dx["workspace"] == lib.nnc_cbmm_grouped_dx_h16_workspace_bytes(m, kdim, ncols) == lib.nnc_cbmm_dx_h16_workspace_bytes(m, kdim, ncols, 1)
        for p in (dx, dc):
            want = _group_fields(p["path"], p, kdim, gr)
            assert {f: p[f] for f in want} == want
            assert p["held"] == (ref.tile_tables(gr) if p["path"] == PATH_MFMA else 0)
            assert p["dtype"] == DT_CODE[dtype]
            if p["path"] == PATH_MFMA:
                assert p["copies"] % p["held"] == 0 and p["copies"] // p["held"] >= 2 and p["lds"] * 2 <= 160 * 1024   # two workgroups a CU
        if 0 < m <= 16 and kdim and ncols:                                                          # the stream plans: the float32 grouped ones, field for field
            fdx, fdc = ops.cbmm_grouped_dx_plan(m, kdim, ncols, k, gr, cus), ops.cbmm_grouped_dc_plan(m, kdim, ncols, k, gr, cus)
            assert dx["path"] == dc["path"] == PATH_STREAM
            assert all(dx[f] == v for f, v in fdx.items()) and all(dc[f] == v for f, v in fdc.items())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits,k", [(2, 3), (4, 16)])
@pytest.mark.parametrize("gr", [32, 96, 128, 4096])
@pytest.mark.parametrize("m,kdim,ncols", SHAPES)
def test_packed_plans_are_the_ungrouped_packed_half_plans_plus_the_group_fields(lib, m, kdim, ncols, gr, bits, k, dtype):
    dt = TDT[dtype]
    G = max(1, -(-kdim // gr))
    for cus in ref.CU_COUNTS:
        dx, dc = ops.cbpk_grouped_dx_h16_plan(dt, m, kdim, ncols, bits, k, gr, cus), ops.cbpk_grouped_dc_h16_plan(dt, m, kdim, ncols, bits, k, gr, cus)
        udx, udc = ops.cbpk_dx_h16_plan(dt, m, kdim, ncols, bits, k, cus), ops.cbpk_dc_h16_plan(dt, m, kdim, ncols, bits, k, cus)
        assert {f: dx[f] for f in udx if f != "lds"} == {f: v for f, v in udx.items() if f != "lds"}
        assert {f: dc[f] for f in udc if f not in ("lds", "workspace")} == {f: v for f, v in udc.items() if f not in ("lds", "workspace")}
        empty = m == 0 or kdim == 0 or ncols == 0
        assert dc["workspace"] == (0 if empty else 64 + 8 * G * k) == lib.nnc_cbpk_grouped_dc_h16_workspace_bytes(m, kdim, ncols, bits, k, gr)
        assert dx["workspace"] == lib.nnc_cbpk_grouped_dx_h16_workspace_bytes(m, kdim, ncols, bits)
        for p, stream_held in ((dx, 4), (dc, 1)):
            want = _group_fields(p["path"], p, kdim, gr)
            assert {f: p[f] for f in want} == want
            assert p["held"] == (ref.tile_tables(gr) if p["path"] == PATH_MFMA else (stream_held if p["path"] == PATH_STREAM else 0))
        images = 2 * 128 * 40 * 2
        if dx["path"] == PATH_MFMA:       # whole tables: 2^bits entries x 32 copies each, and a staging row each
            words = dx["held"] * (1 << bits) * 33
            assert dx["lds"] == ((words + 3) & ~3) * 4 + images and dc["lds"] == images + dc["held"] * k * 64 * 8 and dc["lds"] * 2 <= 160 * 1024
        if 0 < m <= 16 and kdim and ncols:
            fdx, fdc = ops.cbpk_grouped_dx_plan(m, kdim, ncols, bits, k, gr, cus), ops.cbpk_grouped_dc_plan(m, kdim, ncols, bits, k, gr, cus)
            assert all(dx[f] == v for f, v in fdx.items()) and all(dc[f] == v for f, v in fdc.items())


def test_tables_per_tile_are_4_2_1():
    for gr, held in ((32, 4), (96, 2), (128, 1), (64, 2), (160, 2), (256, 1)):
        assert ops.cbmm_grouped_dx_h16_plan(torch.bfloat16, 64, 1000, 200, 16, gr, 256)["held"] == held == ref.tile_tables(gr)
        assert ops.cbpk_grouped_dc_h16_plan(torch.float16, 64, 1000, 200, 4, 16, gr, 256)["held"] == held
        # restated from the rows: no 128-row tile that starts on a multiple of 128 lies in more groups than that
        assert max((min(1000, n0 + 128) - 1) // gr - n0 // gr + 1 for n0 in range(0, 1000, 128)) <= held


def test_the_case_lists_reach_every_cell():
    """{stream, MFMA} x {direct, split} x {bf16, fp16} x {byte, 2 bit, 4 bit} for dx and dc (every case runs with both dtypes; section
    12's stream dc plan never splits m), at the 256 CUs of the device the tests run on and at 80"""
    for cus in (80, 256):
        for dtype in DTYPES:
            dt = TDT[dtype]
            seen = {"dx": set(), "dc": set()}
            for c in ref.CASES:
                a = (c["m"], c["kdim"], c["ncols"], c["k"], c["group_rows"], cus)
                seen["dx"].add(ref.regime_of(ops.cbmm_grouped_dx_h16_plan(dt, *a)))
                seen["dc"].add(ref.regime_of(ops.cbmm_grouped_dc_h16_plan(dt, *a)))
            assert seen == ref.REQUIRED, (cus, dtype)
            for bits in (2, 4):
                seen = {"dx": set(), "dc": set()}
                for c in ref.PACKED_CASES:
                    if c["bits"] != bits:
                        continue
                    a = (c["m"], c["kdim"], c["ncols"], bits, c["k"], c["group_rows"], cus)
                    seen["dx"].add(ref.regime_of(ops.cbpk_grouped_dx_h16_plan(dt, *a)))
                    seen["dc"].add(ref.regime_of(ops.cbpk_grouped_dc_h16_plan(dt, *a)))
                assert seen == ref.REQUIRED, (cus, dtype, bits)
    assert {c["k"] for c in ref.CASES} >= {1, 3, 16, 256}
    assert {(c["bits"], c["k"]) for c in ref.PACKED_CASES} >= {(2, 1), (2, 3), (2, 4), (4, 5), (4, 16)}
    assert {c["m"] for c in ref.CASES} >= {1, 5, 16, 17, 64, 130}
    assert all(gref.groups_of(c) * c["k"] <= 1040 for c in ref.CASES)


def _dx(lib, form, **kw):
    a = dict(g=P, dt=1, m=4, kdim=64, idx=P, bits=4, ncols=16, centers=P, k=16, gr=32, dx=P, dxdt=0, ws=None, ws_bytes=0)
    a.update(kw)
    if form == "byte":
        return lib.nnc_cbmm_grouped_dx_h16(a["g"], a["dt"], a["m"], a["kdim"], a["idx"], a["ncols"], a["centers"], a["k"], a["gr"], a["dx"], a["dxdt"], a["ws"],
                                           a["ws_bytes"], None)
    pb = a.get("pb", lib.nnc_cbpk_pack_bytes(a["kdim"], a["ncols"], a["bits"]) if a["kdim"] >= 0 and a["ncols"] >= 0 and a["bits"] in (2, 4) else 0)
    return lib.nnc_cbpk_grouped_dx_h16(a["g"], a["dt"], a["m"], a["kdim"], a["idx"], pb, a["bits"], a["ncols"], a["centers"], a["k"], a["gr"], a["dx"], a["dxdt"],
                                       a["ws"], a["ws_bytes"], None)


def _dc(lib, form, **kw):
    a = dict(x=P, g=P, dt=1, m=4, kdim=64, idx=P, bits=4, ncols=16, k=16, gr=32, dc=P, f64=1, ws=P, ws_bytes=64 + 8 * 2 * 16)
    a.update(kw)
    if form == "byte":
        return lib.nnc_cbmm_grouped_dc_h16(a["x"], a["g"], a["dt"], a["m"], a["kdim"], a["idx"], a["ncols"], a["k"], a["gr"], a["dc"], a["f64"], a["ws"],
                                           a["ws_bytes"], None)
    pb = a.get("pb", lib.nnc_cbpk_pack_bytes(a["kdim"], a["ncols"], a["bits"]) if a["kdim"] >= 0 and a["ncols"] >= 0 and a["bits"] in (2, 4) else 0)
    return lib.nnc_cbpk_grouped_dc_h16(a["x"], a["g"], a["dt"], a["m"], a["kdim"], a["idx"], pb, a["bits"], a["ncols"], a["k"], a["gr"], a["dc"], a["f64"],
                                       a["ws"], a["ws_bytes"], None)


@pytest.mark.parametrize("form", ["byte", "packed"])
def test_argument_errors_come_back_before_any_hip_call(lib, form):
    def err():
        return lib.nnc_last_error().decode()

    for call in (_dx, _dc):
        for bad in (dict(dt=0), dict(dt=3), dict(m=-1), dict(kdim=-1), dict(ncols=-1), dict(k=0), dict(k=257 if form == "byte" else 17),
                    dict(gr=0), dict(gr=48), dict(gr=-32), dict(m=1 << 41), dict(gr=1 << 41)):
            assert call(lib, form, **bad) == NNC_EINVAL, bad
        assert call(lib, form, dt=0) == NNC_EINVAL and "x_dtype must be NNC_DT_BF16 or NNC_DT_F16" in err()
        assert call(lib, form, gr=48) == NNC_EINVAL and "group_rows must be a positive multiple of 32" in err()
        assert call(lib, form, g=P + 1) == NNC_EINVAL and "aligned to its element size" in err()
        assert call(lib, form, g=None) == NNC_EINVAL and "NULL" in err()
        assert call(lib, form, idx=None) == NNC_EINVAL
    if form == "packed":
        assert _dx(lib, form, bits=3) == NNC_EINVAL and _dc(lib, form, bits=8) == NNC_EINVAL
        assert _dx(lib, form, pb=7) == NNC_EINVAL and "packed_bytes" in err()
        assert _dx(lib, form, idx=P + 4) == NNC_EINVAL
    assert _dx(lib, form, dxdt=2) == NNC_EINVAL and "dx_dtype must be NNC_DT_F32 or x_dtype" in err()
    assert _dx(lib, form, centers=None) == NNC_EINVAL and "centers is NULL" in err()
    assert _dx(lib, form, dx=None) == NNC_EINVAL and "dx is NULL" in err()
    assert _dx(lib, form, dx=P + 2) == NNC_EINVAL and "aligned to its element size" in err()      # (a float32 dx on a 2-byte address)
    assert _dx(lib, form, ws_bytes=-1) == NNC_EINVAL
    big = dict(m=4, kdim=64, ncols=1 << 14)          # sixteen column blocks at m = 4: the stream partials need a workspace
    need = lib.nnc_cbmm_grouped_dx_h16_workspace_bytes(4, 64, 1 << 14) if form == "byte" else lib.nnc_cbpk_grouped_dx_h16_workspace_bytes(4, 64, 1 << 14, 4)
    assert need > 0
    assert _dx(lib, form, ws=P, ws_bytes=need - 1, **big) == NNC_ENOSPACE
    assert _dx(lib, form, ws=None, ws_bytes=need, **big) == NNC_EINVAL and "workspace is NULL" in err()
    assert _dx(lib, form, ws=P + 2, ws_bytes=need, **big) == NNC_EINVAL and "4-byte aligned" in err()
    assert _dc(lib, form, x=P + 1) == NNC_EINVAL and _dc(lib, form, x=None) == NNC_EINVAL
    assert _dc(lib, form, dc=None) == NNC_EINVAL and "dc is NULL" in err()
    assert _dc(lib, form, ws_bytes=64 + 8 * 2 * 16 - 1) == NNC_ENOSPACE
    assert _dc(lib, form, ws=None) == NNC_EINVAL and _dc(lib, form, ws=P + 4) == NNC_EINVAL and "8-byte aligned" in err()
    assert _dc(lib, form, ws_bytes=-1) == NNC_EINVAL
    out = (ctypes.c_int64 * 18)()
    plans = ((lib.nnc_cbmm_grouped_dx_h16_plan, lib.nnc_cbmm_grouped_dc_h16_plan) if form == "byte" else
             (lib.nnc_cbpk_grouped_dx_h16_plan, lib.nnc_cbpk_grouped_dc_h16_plan))
    for plan in plans:
        mid = (16, 32, 256, 0) if form == "byte" else (4, 16, 32, 256)

        def args(dt=1, m=4, cus=None, gr=None, o=out):
            a = list(mid)
            if cus is not None:
                a[2 if form == "byte" else 3] = cus
            if gr is not None:
                a[1 if form == "byte" else 2] = gr
            return (dt, m, 64, 16, *a, o)

        assert plan(*args()) == 0 and out[0] == PATH_STREAM and out[13] == 32
        assert plan(*args(dt=0)) == NNC_EINVAL and plan(*args(m=-1)) == NNC_EINVAL and plan(*args(gr=40)) == NNC_EINVAL
        assert plan(*args(cus=0)) == NNC_EINVAL and "cus < 1" in err()
        assert plan(*args(o=None)) == NNC_EINVAL and "out is NULL" in err()


def test_python_errors_that_need_no_device():
    for fn in (ops.cbmm_grouped_dx_h16_plan, ops.cbmm_grouped_dc_h16_plan):
        with pytest.raises(TypeError, match="bfloat16 or torch.float16"):
            fn(torch.float32, 4, 64, 16, 16, 32, 256)
        with pytest.raises(nat.NncError):
            fn(torch.bfloat16, 4, 64, 16, 16, 48, 256)
    for fn in (ops.cbpk_grouped_dx_h16_plan, ops.cbpk_grouped_dc_h16_plan):
        with pytest.raises(TypeError, match="bfloat16 or torch.float16"):
            fn(torch.float32, 4, 64, 16, 4, 16, 32, 256)
        with pytest.raises(nat.NncError):
            fn(torch.float16, 4, 64, 16, 3, 16, 32, 256)
    half = torch.zeros(4, 64, dtype=torch.float16)
    labels, cen = torch.zeros(64 * 16, dtype=torch.uint8), torch.zeros(2, 16)
    with pytest.raises(TypeError, match="float32 activations"):      # without the keyword the pinned errors stay
        ops.grouped_codebook_linear(half, labels, cen, 64, 16, 32)
    with pytest.raises(TypeError, match="float32 activations"):
        ops.grouped_codebook_linear(half.bfloat16(), labels, cen, 64, 16, 32, half_inputs=False)
    with pytest.raises(TypeError, match="CUDA"):                     # with it a host tensor is still no operand
        ops.grouped_codebook_linear(half, labels, cen, 64, 16, 32, half_inputs=True)
    with pytest.raises(TypeError, match="CUDA"):
        ops.grouped_codebook_matmul_dx(torch.zeros(4, 16, dtype=torch.bfloat16), labels, cen, 64, 16, 32)
    with pytest.raises(TypeError, match="one dtype"):
        ops.grouped_codebook_centroid_grad(half, torch.zeros(4, 16), labels, 16, 64, 16, 32)
    with pytest.raises(TypeError, match="PackedCodes"):
        ops.grouped_packed_codebook_linear(half, labels, cen, 32, half_inputs=True)
    for fn, names in ((ops.grouped_codebook_linear, ("half_inputs",)), (ops.grouped_packed_codebook_linear, ("half_inputs",)),
                      (ops.grouped_codebook_matmul_dx, ("out_dtype",)), (ops.grouped_packed_codebook_matmul_dx, ("out_dtype",)),
                      (compressed.compress_network_trainable_grouped, ("half_inputs",)), (trainer.Trainer.fine_tune_grouped, ("activation_dtype",)),
                      (compressed.TrainableGroupedCompressedDense.__init__, ("half_inputs",)), (compressed.TrainableGroupedCompressedDense.from_dense, ("half_inputs",)),
                      (compressed.TrainableGroupedCompressedDense.from_codes, ("half_inputs",)), (compressed.TrainableGroupedCompressedDense.from_grouped, ("half_inputs",)),
                      (compressed.TrainableGroupedPackedCompressedDense.__init__, ("half_inputs",)),
                      (compressed.TrainableGroupedPackedCompressedDense.from_dense, ("half_inputs",)),
                      (compressed.TrainableGroupedPackedCompressedDense.from_codes, ("half_inputs",)),
                      (compressed.TrainableGroupedPackedCompressedDense.from_grouped, ("half_inputs",)),
                      (compressed.TrainableGroupedPackedCompressedDense.from_grouped_packed, ("half_inputs",))):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == names[0] and params[-1].default in (False, None), fn      # the last keyword, off by default
    for cls in (compressed.TrainableGroupedCompressedDense, compressed.TrainableGroupedPackedCompressedDense):
        assert not hasattr(cls, "half_inputs")                                             # an instance attribute only
