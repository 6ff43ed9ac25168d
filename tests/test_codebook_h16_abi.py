"""CPU checks of the half-precision codebook matmul's C ABI (include/nnc.h, nnc_cbmm_h16*): the plan's invariants at several CU
counts, the coverage of the case list the GPU suite runs (tests/helpers/h16_ref.py), and every argument error coming back before any
HIP call, so none of this needs a device."""
import ctypes
import os
import re

import pytest

from neural_network_compression_amd import _native as nat
from neural_network_compression_amd import build as nbuild
from tests.helpers import h16_ref

NNC_EINVAL, NNC_ENOSPACE = -1, -2
BF16, F16, F32 = nat.DT_BF16, nat.DT_F16, nat.DT_F32


@pytest.fixture(scope="module")
def lib():
    nbuild.build_native()
    return nat.load()


def plan(lib, dt, m, kdim, ncols, lb, k, cus, addr=0):
    out = (ctypes.c_int64 * nat.CBMM_H16_PLAN_LEN)()
    rc = lib.nnc_cbmm_h16_plan(dt, m, kdim, ncols, lb, k, cus, addr, out)
    assert rc == 0, (dt, m, kdim, ncols, lb, k, cus, addr, lib.nnc_last_error())
    return dict(zip(nat.CBMM_H16_PLAN_FIELDS, out))


def test_symbols_header_and_signatures_agree(lib):
    raw = ctypes.CDLL(nat.lib_path())
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nnc.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(nnc_cbmm_h16\w*)\s*\(", code))
    assert declared == {"nnc_cbmm_h16", "nnc_cbmm_h16_workspace_bytes", "nnc_cbmm_h16_plan"}
    for s in declared:
        assert hasattr(raw, s) and s in nat.SIGNATURES, s
    defs = {k: int(v) for k, v in re.findall(r"#define (NNC_\w+) (\d+)", text)}
    assert (defs["NNC_DT_F32"], defs["NNC_DT_BF16"], defs["NNC_DT_F16"]) == (F32, BF16, F16)
    assert defs["NNC_CBMM_MFMA"] == nat.CBMM_MFMA == h16_ref.PATH_MFMA and defs["NNC_CBMM_STREAM"] == h16_ref.PATH_STREAM
    assert defs["NNC_CBMM_H16_PLAN_LEN"] == nat.CBMM_H16_PLAN_LEN == len(nat.CBMM_H16_PLAN_FIELDS)
    assert defs["NNC_CBMM_H16_P_DTYPE"] == nat.CBMM_H16_PLAN_FIELDS.index("dtype") == defs["NNC_CBMM_PLAN_LEN"]
    assert h16_ref.DT_CODE == {"bf16": BF16, "fp16": F16}
    assert lib.nnc_version() == 100


PLAN_MS = list(range(0, 19)) + [64, 128, 129, 4099]
PLAN_KDIMS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 100, 255, 256, 257, 511, 512, 1000, 1001, 2450, 4096, 5003]
PLAN_NCOLS = [1, 7, 63, 64, 65, 128, 129, 300, 1025, 4097, 5000]
PLAN_CUS = [1, 32, 80, 255, 256, 304, 1024]


def test_plan_splits_tiles_and_workspace(lib):
    """splits x rps >= kdim with no empty split; the workspace is the splits' float32 partials and fits the query (which plans for
    256 CUs); splits never shrink as CUs are added and stop growing at 256; stream for m <= 16 and MFMA above; an MFMA split starts
    on a whole k step of 32."""
    for dt, lb in ((BF16, 1), (F16, 2)):
        k = 256 if lb == 1 else 1040
        for m in PLAN_MS:
            for kdim in PLAN_KDIMS:
                for ncols in PLAN_NCOLS:
                    ws = lib.nnc_cbmm_h16_workspace_bytes(m, kdim, ncols, lb)
                    prev = None
                    for cus in PLAN_CUS:
                        p = plan(lib, dt, m, kdim, ncols, lb, k, cus)
                        where = (m, kdim, ncols, lb, cus, p)
                        assert p["dtype"] == dt
                        if m == 0:
                            assert p["path"] == nat.CBMM_NONE and p["splits"] == 0 and p["workspace"] == 0, where
                            continue
                        assert p["path"] == (nat.CBMM_STREAM if m <= 16 else nat.CBMM_MFMA), where
                        s, rps = p["splits"], p["rps"]
                        assert s >= 1 and (s - 1) * rps < kdim <= s * rps, where
                        assert p["workspace"] == (s * m * ncols * 4 if s > 1 else 0), where
                        assert ws >= p["workspace"], where
                        assert p["lds"] <= 64 * 1024, where
                        if p["path"] == nat.CBMM_MFMA:
                            assert p["col_tiles"] == -(-ncols // 128) and p["row_tiles"] == -(-m // 128), where
                            assert s <= 16 and rps % 32 == 0, where
                        if prev is not None:
                            assert s >= prev["splits"], (where, prev)
                        if cus >= 256:
                            assert p == plan(lib, dt, m, kdim, ncols, lb, k, 256), where
                        prev = p


def test_stream_plan_is_the_float32_plan(lib):
    """m <= 16 takes the float32 path's stream plan field for field: the same kernel on half the x bytes."""
    out = (ctypes.c_int64 * nat.CBMM_PLAN_LEN)()
    for lb, k in ((1, 256), (2, 257), (2, 1040)):
        for m in range(1, 17):
            for kdim, ncols, addr in ((257, 64, 0), (1001, 63, 3), (5000, 300, 2)):
                assert lib.nnc_cbmm_plan(m, kdim, ncols, lb, k, 256, addr, out) == 0
                p = plan(lib, F16, m, kdim, ncols, lb, k, 256, addr)
                assert [p[f] for f in nat.CBMM_PLAN_FIELDS] == list(out), (m, kdim, ncols, lb)


@pytest.mark.parametrize("cus", [80, 256, 304])
def test_cases_cover_every_regime(lib, cus):
    """The list the GPU suite runs hits {stream, MFMA} x {uint8, uint16} x {direct, split} x {bf16, fp16}, and the larger kdims
    split at every m."""
    hit = set()
    for c in h16_ref.CASES:
        for dtype in h16_ref.DTYPES:
            p = plan(lib, h16_ref.DT_CODE[dtype], c["m"], c["kdim"], c["ncols"], c["lb"], c["k"], cus, 4096 + c["off"] * c["lb"])
            hit.add(h16_ref.regime_of(c, p, dtype))
            if c["kdim"] in h16_ref.MUST_SPLIT_KDIMS:
                assert p["splits"] > 1, (c, p)
    assert hit == h16_ref.required_regimes(), sorted(h16_ref.required_regimes() - hit)
    assert {c["m"] for c in h16_ref.CASES} == set(h16_ref.MS) and {c["kdim"] for c in h16_ref.CASES} == set(h16_ref.KDIMS)
    assert {c["ncols"] for c in h16_ref.CASES} == set(h16_ref.NCOLS)
    assert {c["off"] % 2 for c in h16_ref.CASES} == {0, 1}


# a fake, never dereferenced address: the argument checks return before anything touches it
P = 0x1000


def call(lib, x=P, dt=BF16, m=4, kdim=8, labels=P, lb=1, ncols=16, centers=P, k=16, bias=None, relu=0, y=P, ydt=None, ws=None, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.nnc_cbmm_h16_workspace_bytes(m, kdim, ncols, lb) if m >= 0 and kdim >= 0 and ncols >= 0 else 0
    return lib.nnc_cbmm_h16(x, dt, m, kdim, labels, lb, ncols, centers, k, bias, relu, y, dt if ydt is None else ydt, ws, ws_bytes, None)


@pytest.mark.parametrize("kw", [
    dict(x=None), dict(labels=None), dict(centers=None), dict(y=None),
    dict(m=-1), dict(kdim=-1), dict(ncols=-1),
    dict(k=0), dict(k=-3), dict(k=1041, lb=2),
    dict(lb=0), dict(lb=3), dict(k=257, lb=1),
    dict(dt=F32), dict(dt=3), dict(dt=-1),
    dict(dt=BF16, ydt=F16), dict(dt=F16, ydt=BF16), dict(ydt=7),
    dict(x=P + 1), dict(y=P + 1), dict(y=P + 2, ydt=F32),
    dict(ws_bytes=-1),
])
def test_bad_arguments_are_einval_without_a_device(lib, kw):
    assert call(lib, **kw) == NNC_EINVAL
    assert lib.nnc_last_error()


def test_short_workspace_is_enospace_without_a_device(lib):
    for m in (1, 40):
        kdim, ncols = 5000, 300
        need = lib.nnc_cbmm_h16_workspace_bytes(m, kdim, ncols, 1)
        assert need > 0 and need % (4 * m * ncols) == 0
        assert call(lib, m=m, kdim=kdim, ncols=ncols, ws=P, ws_bytes=need - 1) == NNC_ENOSPACE
        assert call(lib, m=m, kdim=kdim, ncols=ncols, ws=None, ws_bytes=need) == NNC_EINVAL    # big enough, but NULL


def test_limits_and_noops_are_accepted(lib):
    assert call(lib, m=0, k=256, lb=1) == 0
    assert call(lib, m=0, k=nat.NNC_KMAX, lb=2, dt=F16, ydt=F32) == 0
    assert call(lib, ncols=0, x=None, labels=None, y=None) == 0
    assert call(lib, m=0, x=P + 2, y=P + 2) == 0                      # 2-byte aligned x and half y
    assert lib.nnc_cbmm_h16_workspace_bytes(-1, 10, 10, 1) == 0 and lib.nnc_cbmm_h16_workspace_bytes(1, 10, 10, 3) == 0


def test_plan_degenerate_shapes_and_errors(lib):
    assert plan(lib, BF16, 0, 10, 10, 1, 4, 256)["path"] == nat.CBMM_NONE
    assert plan(lib, F16, 3, 10, 0, 1, 4, 256)["path"] == nat.CBMM_NONE
    p = plan(lib, F16, 3, 0, 10, 1, 4, 256)
    assert p["path"] == nat.CBMM_BIAS and p["splits"] == 0 and p["workspace"] == 0
    out = (ctypes.c_int64 * nat.CBMM_H16_PLAN_LEN)()
    for args in ((F32, 1, 1, 1, 1, 1, 1), (BF16, -1, 1, 1, 1, 1, 1), (BF16, 1, 1, 1, 3, 1, 1), (F16, 1, 1, 1, 1, 257, 1), (F16, 1, 1, 1, 1, 1, 0)):
        assert lib.nnc_cbmm_h16_plan(*args, 0, out) == NNC_EINVAL and lib.nnc_last_error()
    assert lib.nnc_cbmm_h16_plan(BF16, 1, 1, 1, 1, 1, 1, 0, None) == NNC_EINVAL


def test_ops_plan_wrapper_takes_torch_dtypes():
    torch = pytest.importorskip("torch")
    from neural_network_compression_amd import ops

    with pytest.raises(TypeError):
        ops.cbmm_h16_plan(torch.float32, 1, 1, 1, 1, 1, 1)
    assert ops.cbmm_h16_plan(torch.bfloat16, 17, 300, 50, 1, 17, 256)["path"] == nat.CBMM_MFMA
