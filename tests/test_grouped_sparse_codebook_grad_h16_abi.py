"""CPU checks of the C ABI of the grouped bitmap-sparse backward pass on bf16 / fp16 activations (include/nnc_cbspgrad_grouped_h16.h,
nnc_cbsp_grouped_dx_h16 / _dc_h16): the argument errors (returned before any HIP call, so none of this needs a
device), the plans against the ungrouped sparse half plans and the group fields, and the Python doors."""
import ctypes
import inspect

import pytest
import torch

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from neural_network_compression_amd import compressed, ops
from neural_network_compression_amd.common import trainer

NNC_EINVAL, NNC_ENOSPACE = -1, -2
PATH_STREAM, PATH_MFMA = 1, 5
P = 0x1000   # a fake, never dereferenced, 256-byte aligned address


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def _dx(lib, **kw):
    a = dict(g=P, dt=1, m=4, kdim=64, packed=P, ncols=16, zs=P, nnz=10, centers=P, k=16, gr=32, dx=P, dxdt=0, ws=P)
    a.update(kw)
    pb = a.get("pb", lib.nnc_cbsp_pack_bytes(max(a["kdim"], 0), max(a["ncols"], 0), 1, max(a["nnz"], 0)))
    wb = a.get("ws_bytes", lib.nnc_cbsp_grouped_dx_h16_workspace_bytes(a["m"], a["kdim"], a["ncols"]))
    return lib.nnc_cbsp_grouped_dx_h16(a["g"], a["dt"], a["m"], a["kdim"], a["packed"], pb, a["ncols"], a["zs"], a["nnz"], a["centers"], a["k"], a["gr"],
                                       a["dx"], a["dxdt"], a["ws"], wb, None)


def _dc(lib, **kw):
    a = dict(x=P, g=P, dt=1, m=4, kdim=64, packed=P, ncols=16, zs=P, nnz=10, k=16, gr=32, dc=P, f64=1, ws=P, ws_bytes=64 + 8 * 2 * 16)
    a.update(kw)
    pb = a.get("pb", lib.nnc_cbsp_pack_bytes(max(a["kdim"], 0), max(a["ncols"], 0), 1, max(a["nnz"], 0)))
    return lib.nnc_cbsp_grouped_dc_h16(a["x"], a["g"], a["dt"], a["m"], a["kdim"], a["packed"], pb, a["ncols"], a["zs"], a["nnz"], a["k"], a["gr"], a["dc"],
                                       a["f64"], a["ws"], a["ws_bytes"], None)


def test_argument_errors_come_back_before_any_hip_call(lib):
    def err():
        return lib.nnc_last_error().decode()

    for call in (_dx, _dc):
        for bad in (dict(dt=0), dict(dt=3), dict(m=-1), dict(kdim=-1), dict(ncols=-1), dict(k=0), dict(k=257), dict(gr=0), dict(gr=48), dict(nnz=-1),
                    dict(nnz=64 * 16 + 1), dict(pb=8), dict(packed=None), dict(packed=P + 16), dict(zs=None), dict(g=None), dict(g=P + 1)):
            assert call(lib, **bad) == NNC_EINVAL, bad
        assert call(lib, dt=0) == NNC_EINVAL and "x_dtype must be NNC_DT_BF16 or NNC_DT_F16" in err()
        assert call(lib, gr=48) == NNC_EINVAL and "group_rows must be a positive multiple of 32" in err()
    assert _dx(lib, dxdt=2) == NNC_EINVAL and "dx_dtype must be NNC_DT_F32 or x_dtype" in err()
    assert _dx(lib, centers=None) == NNC_EINVAL and "centers is NULL" in err()
    assert _dx(lib, dx=None) == NNC_EINVAL and _dx(lib, dx=P + 2) == NNC_EINVAL and "aligned to its element size" in err()
    need = lib.nnc_cbsp_grouped_dx_h16_workspace_bytes(4, 64, 16)
    assert need == 4 * 64 * 4 + 4 * 4                      # one column block: still a block of partials, then the row sums
    assert _dx(lib, ws_bytes=need - 1) == NNC_ENOSPACE and _dx(lib, ws=None) == NNC_EINVAL and _dx(lib, ws=P + 2) == NNC_EINVAL
    assert _dc(lib, x=P + 1) == NNC_EINVAL and _dc(lib, x=None) == NNC_EINVAL and _dc(lib, dc=None) == NNC_EINVAL and "dc is NULL" in err()
    assert _dc(lib, ws_bytes=64 + 8 * 2 * 16 - 1) == NNC_ENOSPACE and _dc(lib, ws=P + 4) == NNC_EINVAL and "8-byte aligned" in err()
    out = (ctypes.c_int64 * 18)()
    for plan in (lib.nnc_cbsp_grouped_dx_h16_plan, lib.nnc_cbsp_grouped_dc_h16_plan):
        assert plan(1, 4, 64, 16, 16, 32, 256, out) == 0 and out[0] == PATH_STREAM and out[13] == 32
        assert plan(0, 4, 64, 16, 16, 32, 256, out) == NNC_EINVAL and plan(1, 4, 64, 16, 16, 40, 256, out) == NNC_EINVAL
        assert plan(1, 4, 64, 16, 16, 32, 0, out) == NNC_EINVAL and "cus < 1" in err()
        assert plan(1, 4, 64, 16, 16, 32, 256, None) == NNC_EINVAL and "out is NULL" in err()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("gr,held", [(32, 4), (96, 2), (128, 1), (4096, 1)])
@pytest.mark.parametrize("m,kdim,ncols", [(1, 300, 50), (16, 200, 300), (17, 300, 130), (130, 200, 50), (4096, 4096, 4096), (0, 50, 60), (20, 0, 60), (20, 50, 0)])
def test_plans_are_the_ungrouped_sparse_half_plans_plus_the_group_fields(lib, m, kdim, ncols, gr, held, dt):
    k, G = 16, max(1, -(-kdim // gr))
    for cus in (80, 256):
        dx, dc = ops.cbsp_grouped_dx_h16_plan(dt, m, kdim, ncols, k, gr, cus), ops.cbsp_grouped_dc_h16_plan(dt, m, kdim, ncols, k, gr, cus)
        udx, udc = ops.cbsp_dx_h16_plan(dt, m, kdim, ncols, 1, k, cus), ops.cbsp_dc_h16_plan(dt, m, kdim, ncols, 1, k, cus)
        assert len(dx) == len(dc) == 18 == nat.CBGRAD_GROUPED_H16_PLAN_LEN
        assert {f: v for f, v in dx.items() if f in udx and f != "workspace"} == {f: v for f, v in udx.items() if f != "workspace"}
        assert {f: v for f, v in dc.items() if f in udc and f != "workspace"} == {f: v for f, v in udc.items() if f != "workspace"}
        product = m > 0 and kdim > 0 and ncols > 0
        assert dx["path"] == dc["path"] or not product
        assert (dx["path"] == PATH_MFMA) == (dc["path"] == PATH_MFMA) == (m > 16 and product)       # the MFMA tile exactly above 16 rows
        assert dc["workspace"] == (64 + 8 * G * k if product else 0) == lib.nnc_cbsp_grouped_dc_h16_workspace_bytes(m, kdim, ncols, k, gr)
        assert dx["workspace"] == lib.nnc_cbsp_grouped_dx_h16_workspace_bytes(m, kdim, ncols)
        if dx["path"] == PATH_MFMA:
            assert dx["workspace"] == udx["workspace"]
            byte = ops.cbmm_grouped_dx_h16_plan(dt, m, kdim, ncols, k, gr, cus), ops.cbmm_grouped_dc_h16_plan(dt, m, kdim, ncols, k, gr, cus)
            for p, b in zip((dx, dc), byte):   # the byte grouped kernels' tiles, splits and LDS
                assert all(p[f] == b[f] for f in ("lds", "splits", "col_tiles", "row_tiles", "copies", "held", "max_groups_per_workgroup")), p
        elif dx["path"] == PATH_STREAM:
            assert dx["workspace"] == (max(dx["splits"], 1) * m * kdim * 4 + 255) // 256 * 256 + 4 * m
        for p in (dx, dc):
            assert (p["reserved"], p["group_rows"], p["groups"]) == (0, gr, -(-kdim // gr) if kdim else 0)
            assert p["held"] == (held if p["path"] == PATH_MFMA else 0) and p["dtype"] == {torch.bfloat16: 1, torch.float16: 2}[dt]
            assert p["rows_per_group"] == (0 if p["path"] != PATH_STREAM else -(-kdim // p["row_tiles"]))


def test_the_python_doors():
    for fn in (ops.grouped_sparse_codebook_matmul_dx, ops.grouped_sparse_codebook_centroid_grad, ops.grouped_sparse_codebook_linear,
               compressed.TrainableGroupedSparseCompressedDense.__init__, compressed.TrainableGroupedSparseCompressedDense.from_dense,
               compressed.TrainableGroupedSparseCompressedDense.from_codes, compressed.TrainableGroupedSparseCompressedDense.from_grouped,
               compressed.TrainableGroupedSparseCompressedDense.from_grouped_sparse):
        assert inspect.signature(fn).parameters["half_inputs"].default is False, fn
    assert inspect.signature(ops.grouped_sparse_codebook_matmul_dx).parameters["out_dtype"].default is None
    for fn in (compressed.compress_network_trainable_grouped, trainer.Trainer.fine_tune_grouped):
        assert inspect.signature(fn).parameters["sparse_half_inputs"].default is False, fn
    assert not hasattr(compressed.TrainableGroupedSparseCompressedDense, "half_inputs")   # an instance attribute only
    with pytest.raises(ValueError, match="sparse_half_inputs=True needs sparse"):
        compressed.compress_network_trainable_grouped(None, {}, sparse_half_inputs=True)
    with pytest.raises(ValueError, match="sparse_half_inputs=True needs sparse"):          # the trainer's door agrees
        trainer.Trainer.fine_tune_grouped(None, None, None, 1, sparse_half_inputs=True, activation_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="sparse needs half_inputs=False"):              # without the keyword the old refusals stay
        compressed.compress_network_trainable_grouped(None, {}, sparse=True, half_inputs=True)
    with pytest.raises(ValueError, match="sparse needs activation_dtype=None"):
        trainer.Trainer.fine_tune_grouped(None, None, None, 1, sparse=True, activation_dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="bfloat16 or torch.float16"):
        ops.cbsp_grouped_dx_h16_plan(torch.float32, 4, 64, 16, 16, 32, 256)
    half = torch.zeros(4, 16, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="float32 activations"):
        ops.grouped_sparse_codebook_matmul_dx(half, None, None)
    with pytest.raises(TypeError, match="CUDA"):                                         # with the keyword a host tensor is still no operand
        ops.grouped_sparse_codebook_matmul_dx(half, None, None, half_inputs=True)
