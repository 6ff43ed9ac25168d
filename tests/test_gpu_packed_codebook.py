"""Layers of at most 16 centres run from 2- and 4-bit packed indices on the GPU (ops.pack_codes / ops.packed_codebook_matmul,
csrc/nnc_cbpk.hip, compressed.Packed*; run with -m gpu).

The pack equals the NumPy reference of the layout (tests/helpers/packed_ref.py) byte for byte; every regime of the plan
(nnc_cbpk_plan) is hit and, on exact data, gives the float64 product bit for bit -- and therefore ops.codebook_matmul on the
unpacked labels bit for bit; fitted layers stay within the float32 bound the byte path is held to; then the conventions (index
>= K reads 0, NaN through ReLU, Inf * 0), the edge sizes, the Conv2D, the LeNets through the Trainer and the stored form, the
footprint and the per-layer selection of the form."""
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import packed_ref  # noqa: E402
from tests.helpers.cbmm_ref import assert_exact, matmul64, relu_like_torch  # noqa: E402
from tests.helpers.packed_ref import PACKED_REGIME_CASES  # noqa: E402
from tests.test_gpu_codebook_matmul import _check_bound, _conv_ref, _fitted, _inputs, _trainer  # noqa: E402

SENTINEL = 0x7FA5A5A5    # a quiet NaN whose payload neither the inputs nor the kernels' own NaNs carry
Y_PAD, WS_PAD = 37, 64


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, compressed, ops, pipeline

    L = _native.load()
    _, cus = ops.device_info()
    assert cus >= 1
    return SimpleNamespace(L=L, ops=ops, cus=cus, compressed=compressed, pipeline=pipeline)


def _dev_f32(host, view=False):
    host = np.ascontiguousarray(host, dtype=np.float32)
    if not view:
        return torch.from_numpy(host).cuda()
    buf = torch.zeros(host.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(host.ravel()).cuda()
    return buf[1:].view(host.shape)


def _dev_labels(lab, lb, off=0):
    dt = torch.uint8 if lb == 1 else torch.int16
    host = lab.astype(np.uint8) if lb == 1 else lab.astype(np.uint16).view(np.int16)
    buf = torch.zeros(off + host.size + 16, dtype=dt, device="cuda")
    buf[off: off + host.size] = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    return buf[off: off + host.size]


def _sentinel(words):
    return torch.full((words,), SENTINEL, dtype=torch.int32, device="cuda")


def _call(env, x, m, codes, centers, bias, relu):
    """nnc_cbpk_f32 into sentinel-framed y and workspace (exactly the queried size); checks the frames; returns y (device)."""
    L = env.L
    kdim, ncols = codes.kdim, codes.ncols
    ws_bytes = int(L.nnc_cbpk_workspace_bytes(m, kdim, ncols, codes.bits))
    assert ws_bytes % 4 == 0
    mn = m * ncols
    ybuf, wsbuf = _sentinel(mn + 2 * Y_PAD), _sentinel(ws_bytes // 4 + 2 * WS_PAD)
    y = ybuf[Y_PAD: Y_PAD + mn]
    ws_ptr = wsbuf[WS_PAD:].data_ptr() if ws_bytes else None
    env.ops.nat.check(L.nnc_cbpk_f32(x.data_ptr(), m, kdim, codes.packed.data_ptr(), codes.nbytes, codes.bits, ncols, centers.data_ptr(),
                                     centers.numel(), None if bias is None else bias.data_ptr(), int(relu), y.data_ptr(), ws_ptr, ws_bytes,
                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((ybuf[:Y_PAD] == SENTINEL).all()) and bool((ybuf[Y_PAD + mn:] == SENTINEL).all()), "a store outside y"
    assert bool((wsbuf[:WS_PAD] == SENTINEL).all()) and bool((wsbuf[WS_PAD + ws_bytes // 4:] == SENTINEL).all()), "a store outside the workspace"
    assert not bool((y == SENTINEL).any()), "an output left unwritten"
    return y.view(torch.float32).view(m, ncols)


# ------------------------------------------------------------------ pack / unpack
@pytest.mark.parametrize("bits", [2, 4])
@pytest.mark.parametrize("lb", [1, 2])
def test_pack_equals_the_numpy_reference_and_unpack_inverts_it(env, bits, lb):
    """uint8 and uint16 labels at storage offsets 0..3, rows that fill their 16-byte groups and rows that do not: the buffer is
    the reference's byte for byte (padding included: it is filled with ones first), and unpack returns the labels in both widths."""
    ops, L = env.ops, env.L
    rng = np.random.RandomState(10 * bits + lb)
    for kdim, ncols in ((1, 1), (3, 7), (9, 31), (5, 32), (5, 33), (4, 64), (7, 50), (3, 1027), (2, 1040), (300, 100), (0, 5), (5, 0)):
        for off in range(4):
            k = (1 << bits) if off % 2 == 0 else max(1, (1 << bits) - 1)
            lab = rng.randint(0, k, size=kdim * ncols)
            lab_t = _dev_labels(lab, lb, off)
            assert lab_t.storage_offset() == off
            codes = ops.pack_codes(lab_t, kdim, ncols, k, bits)
            want = packed_ref.pack(lab, kdim, ncols, bits)
            assert codes.bits == bits and codes.k == k and codes.nbytes == want.size == kdim * packed_ref.row_bytes(ncols, bits)
            assert codes.packed.data_ptr() % 256 == 0
            assert np.array_equal(codes.packed.cpu().numpy(), want), (kdim, ncols, off)
            # the pack writes the padding itself: a buffer of ones gives the same bytes
            buf = torch.full((max(1, want.size),), 0xFF, dtype=torch.uint8, device="cuda")[: want.size]
            bad = torch.full((1,), 77, dtype=torch.int32, device="cuda")
            ops.nat.check(L.nnc_cbpk_pack(lab_t.data_ptr(), lb, kdim, ncols, bits, buf.data_ptr(), want.size, bad.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream))
            assert np.array_equal(buf.cpu().numpy(), want) and int(bad.item()) == 0
            assert np.array_equal(codes.to_dense().cpu().numpy(), lab.astype(np.uint8))
            out16 = torch.full((kdim * ncols + 1,), -1, dtype=torch.int16, device="cuda")
            ops.nat.check(L.nnc_cbpk_unpack(codes.packed.data_ptr(), codes.nbytes, bits, kdim, ncols, out16[1:].data_ptr(), 2,
                                            torch.cuda.current_stream().cuda_stream))
            assert np.array_equal(out16[1:].cpu().numpy(), lab.astype(np.int16)) and int(out16[0]) == -1
    assert ops.pack_codes(_dev_labels(np.zeros(6), 1), 2, 3, 3).bits == 2 and ops.pack_codes(_dev_labels(np.zeros(6), 1), 2, 3, 5).bits == 4


@pytest.mark.parametrize("lb", [1, 2])
def test_an_out_of_range_label_raises_and_is_counted(env, lb):
    ops, L = env.ops, env.L
    rng = np.random.RandomState(3)
    for bits, kdim, ncols in ((2, 7, 33), (4, 300, 100)):
        lab = rng.randint(0, 1 << bits, size=kdim * ncols)
        where = rng.choice(lab.size, size=5, replace=False)
        lab[where] = (1 << bits) + rng.randint(0, 200 if lb == 1 else 60000, size=5)
        lab_t = _dev_labels(lab, lb, 1)
        with pytest.raises(ValueError, match="5 labels"):
            ops.pack_codes(lab_t, kdim, ncols, 1 << bits, bits)
        nb = packed_ref.row_bytes(ncols, bits) * kdim
        buf = torch.empty(nb, dtype=torch.uint8, device="cuda")
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        ops.nat.check(L.nnc_cbpk_pack(lab_t.data_ptr(), lb, kdim, ncols, bits, buf.data_ptr(), nb, bad.data_ptr(), torch.cuda.current_stream().cuda_stream))
        assert int(bad.item()) == 5
        assert np.array_equal(buf.cpu().numpy(), packed_ref.pack(lab & ((1 << bits) - 1), kdim, ncols, bits))   # stored as its low bits
    with pytest.raises(ValueError):
        ops.pack_codes(lab_t, kdim, ncols, 17)


# ------------------------------------------------------------------ every regime
def test_the_cases_hit_every_regime_at_this_device(env):
    hit = set()
    for c in PACKED_REGIME_CASES:
        hit |= packed_ref.regime_of(c, env.ops.cbpk_plan(c["m"], c["kdim"], c["ncols"], c["bits"], c["k"], env.cus))
    assert hit == packed_ref.required_regimes(), sorted(packed_ref.required_regimes() - hit, key=str)


@pytest.mark.parametrize("ci", range(len(PACKED_REGIME_CASES)), ids=[packed_ref.case_id(c) for c in PACKED_REGIME_CASES])
def test_regime_case(env, ci):
    ops = env.ops
    c = PACKED_REGIME_CASES[ci]
    m, kdim, ncols, bits, k = c["m"], c["kdim"], c["ncols"], c["bits"], c["k"]
    rng = np.random.RandomState(9000 + ci)
    lab = rng.randint(0, k, size=kdim * ncols)
    lab_t = _dev_labels(lab, 1, ci % 4)
    codes = ops.pack_codes(lab_t, kdim, ncols, k, bits)
    assert np.array_equal(codes.packed.cpu().numpy(), packed_ref.pack(lab, kdim, ncols, bits))

    # exact data: the float64 result bit for bit in all four bias / ReLU combinations, the byte path's bits, the same bits twice
    x = rng.randint(-8, 9, size=(m, kdim)).astype(np.float32)
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    bias = rng.randint(-50, 51, size=ncols).astype(np.float32)
    w = cen[lab].reshape(kdim, ncols)
    assert_exact(x, w, bias)
    x_t, cen_t = _dev_f32(x, c["x_view"]), _dev_f32(cen)
    bias_t = _dev_f32(bias, c["bias_view"])
    for use_bias in (False, True):
        want = matmul64(x, w, bias if use_bias else None)
        for relu in (False, True):
            y = _call(env, x_t, m, codes, cen_t, bias_t if use_bias else None, relu)
            ref = (relu_like_torch(want) if relu else want).astype(np.float32)
            assert np.array_equal(y.cpu().numpy(), ref), (c, use_bias, relu)
            yb = ops.codebook_matmul(x_t, codes.to_dense(), cen_t, kdim, ncols, bias=bias_t if use_bias else None, relu=relu)
            assert torch.equal(y.view(torch.int32), yb.view(torch.int32)), (c, use_bias, relu)
            assert torch.equal(ops.packed_codebook_matmul(x_t, codes, cen_t, bias=bias_t if use_bias else None, relu=relu).view(torch.int32),
                               y.view(torch.int32))
    y2 = _call(env, x_t, m, codes, cen_t, bias_t, True)
    assert torch.equal(_call(env, x_t, m, codes, cen_t, bias_t, True).view(torch.int32), y2.view(torch.int32))

    # float data: within 2 kdim 2^-24 (|x| @ |W| + |b|); the same bits twice
    xf = rng.standard_normal((m, kdim)).astype(np.float32)
    cf = rng.standard_normal(k).astype(np.float32)
    bf = rng.standard_normal(ncols).astype(np.float32) if c["bias"] else None
    xf_t, cf_t = _dev_f32(xf, c["x_view"]), _dev_f32(cf)
    bf_t = None if bf is None else _dev_f32(bf, c["bias_view"])
    y = _call(env, xf_t, m, codes, cf_t, bf_t, False)
    _check_bound(y.cpu().numpy(), xf, cf[lab].reshape(kdim, ncols), bf)
    assert torch.equal(y.view(torch.int32), _call(env, xf_t, m, codes, cf_t, bf_t, False).view(torch.int32))


# ------------------------------------------------------------------ fitted layers
FIT_SHAPES = [(784, 300), (300, 100), (100, 10), (2450, 256), (4096, 4096), (5000, 5000)]
FITS = [(4, "linear", 16, 4), (2, "linear", 4, 2), (2, "density", 5, 4)]   # (bits of the fit, init, K, width of the packed form)


@pytest.mark.parametrize("fit_bits,mode,want_k,want_bits", FITS)
@pytest.mark.parametrize("shape", FIT_SHAPES)
def test_fitted_layers_within_the_float32_bound_and_deterministic(env, shape, fit_bits, mode, want_k, want_bits):
    ops = env.ops
    model, _ = _fitted(env.pipeline, shape, fit_bits, mode, 4242 + shape[0])
    kdim, ncols = shape
    cen = torch.from_numpy(np.ascontiguousarray(model.cluster_centers_.ravel())).cuda()
    lab = model.labels_compact_
    assert cen.numel() == want_k and lab.dtype == torch.uint8
    codes = ops.pack_codes(lab, kdim, ncols, cen.numel())
    assert codes.bits == want_bits and codes.nbytes == kdim * packed_ref.row_bytes(ncols, want_bits)
    assert torch.equal(codes.to_dense(), lab.reshape(-1))
    w = ops.gather(cen, lab).cpu().numpy().reshape(kdim, ncols)
    rng = np.random.RandomState(kdim)
    for m in (1, 16, 256):
        x = rng.rand(m, kdim).astype(np.float32)
        xt = torch.from_numpy(x).cuda()
        y = ops.packed_codebook_matmul(xt, codes, cen)
        _check_bound(y.cpu().numpy(), x, w)
        y2 = ops.packed_codebook_matmul(xt, codes, cen)
        assert torch.equal(y.view(torch.int32), y2.view(torch.int32))   # the same bits, twice


@pytest.mark.parametrize("fit_bits,mode", [(4, "linear"), (2, "linear")])
def test_no_float32_weight_matrix_is_materialized(env, fit_bits, mode):
    ops = env.ops
    model, (kdim, ncols) = _fitted(env.pipeline, (5000, 5000), fit_bits, mode, 4242 + 5000)
    cen = torch.from_numpy(np.ascontiguousarray(model.cluster_centers_.ravel())).cuda()
    codes = ops.pack_codes(model.labels_compact_, kdim, ncols, cen.numel())
    for m in (1, 16):
        x = torch.rand(m, kdim, device="cuda")
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = ops.packed_codebook_matmul(x, codes, cen)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - base
        assert grown < 2 * kdim * ncols, grown
        del y


# ------------------------------------------------------------------ conventions
def test_an_index_at_or_above_k_reads_zero(env):
    """K = 5 in the 4-bit form with stored 9s (and 5s, 15s): those weights are 0, in the stream and in the tiled kernel."""
    ops = env.ops
    rng = np.random.RandomState(5)
    kdim, ncols, k = 300, 77, 5
    lab = rng.randint(0, k, size=kdim * ncols)
    lab[rng.choice(lab.size, size=2000, replace=False)] = rng.choice([9, 5, 15], size=2000)
    cen = (rng.randint(1, 17, size=k) / 4.0).astype(np.float32)
    w = np.where(lab < k, cen[np.minimum(lab, k - 1)], 0.0).reshape(kdim, ncols)
    buf = torch.from_numpy(packed_ref.pack(lab, kdim, ncols, 4)).cuda()
    assert buf.data_ptr() % 16 == 0
    codes = ops.PackedCodes(buf, kdim, ncols, 4, k)
    assert np.array_equal(codes.to_dense().cpu().numpy(), lab.astype(np.uint8))
    for m in (3, 16, 40):
        x = rng.randint(-8, 9, size=(m, kdim)).astype(np.float32)
        assert_exact(x, w)
        y = ops.packed_codebook_matmul(torch.from_numpy(x).cuda(), codes, torch.from_numpy(cen).cuda())
        assert np.array_equal(y.cpu().numpy(), matmul64(x, w).astype(np.float32)), m
        yb = ops.codebook_matmul(torch.from_numpy(x).cuda(), torch.from_numpy(lab.astype(np.uint8)).cuda(), torch.from_numpy(cen).cuda(), kdim, ncols)
        assert torch.equal(y.view(torch.int32), yb.view(torch.int32))


# (m, kdim, ncols, bits, k, path, split)
NONFINITE = [(3, 20, 77, 4, 16, 1, False), (5, 700, 50, 2, 4, 1, True), (16, 600, 33, 4, 5, 1, True), (40, 100, 129, 2, 3, 2, False),
             (17, 300, 50, 4, 16, 2, True)]


@pytest.mark.parametrize("m,kdim,ncols,bits,k,path,split", NONFINITE)
def test_nonfinite_inputs_behave_as_in_the_byte_path(env, m, kdim, ncols, bits, k, path, split):
    """NaN and +-Inf in x, NaN in the bias; Inf against the centre that is exactly 0 gives NaN (nothing is skipped); the fused
    ReLU maps -Inf to 0 and keeps NaN.  The float64 result, and the byte path's bits."""
    ops = env.ops
    rng = np.random.RandomState(m * 1000 + kdim)
    lab = rng.randint(0, k, size=(kdim, ncols))
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    cen[0] = 0.0
    lab[2, ::3] = 0
    x = rng.randint(-8, 9, size=(m, kdim)).astype(np.float32)
    x[0, 1] = np.nan
    x[1, 2] = np.inf
    x[m - 1, 5] = -np.inf
    x[m - 1, kdim - 1] = np.inf
    x[2, 7] = -np.inf
    bias = rng.randint(-50, 51, size=ncols).astype(np.float32)
    bias[4] = np.nan
    w = cen[lab]
    assert_exact(np.where(np.isfinite(x), x, 0), w, np.where(np.isfinite(bias), bias, 0))
    lab_t = _dev_labels(lab.ravel(), 1)
    codes = ops.pack_codes(lab_t, kdim, ncols, k, bits)
    p = ops.cbpk_plan(m, kdim, ncols, bits, k, env.cus)
    assert p["path"] == path and (p["splits"] > 1) == split, p
    want = matmul64(x, w, bias)
    assert np.isnan(want).any() and np.isposinf(want).any()
    assert np.isnan(want[1, ::3]).all()                      # +Inf times the exact 0 centre
    x_t, cen_t, bias_t = _dev_f32(x), _dev_f32(cen), _dev_f32(bias)
    for relu in (False, True):
        y = _call(env, x_t, m, codes, cen_t, bias_t, relu)
        ref = (relu_like_torch(want) if relu else want).astype(np.float32)
        got = y.cpu().numpy()
        assert np.array_equal(got, ref, equal_nan=True), (relu, np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[:5])
        yb = ops.codebook_matmul(x_t, lab_t, cen_t, kdim, ncols, bias=bias_t, relu=relu).cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(yb)) and np.array_equal(got[~np.isnan(got)], yb[~np.isnan(yb)])


def test_edge_sizes_and_argument_checks(env):
    ops = env.ops
    cen = torch.arange(4, dtype=torch.float32, device="cuda")
    bias = torch.tensor([1.0, -2.0, 3.0], device="cuda")
    empty = torch.empty(0, dtype=torch.uint8, device="cuda")
    for bits in (2, 4):
        c0 = ops.pack_codes(empty, 0, 3, 4, bits)                                   # kdim = 0: y = bias, or 0
        assert c0.nbytes == 0
        assert torch.equal(ops.packed_codebook_matmul(torch.empty(5, 0, device="cuda"), c0, cen, bias=bias), bias.expand(5, 3))
        assert torch.equal(ops.packed_codebook_matmul(torch.empty(5, 0, device="cuda"), c0, cen), torch.zeros(5, 3, device="cuda"))
        assert torch.equal(ops.packed_codebook_matmul(torch.empty(5, 0, device="cuda"), c0, cen, bias=-bias, relu=True),
                           torch.relu(-bias).expand(5, 3))
        c7 = ops.pack_codes(torch.zeros(21, dtype=torch.uint8, device="cuda"), 7, 3, 4, bits)
        assert ops.packed_codebook_matmul(torch.empty(0, 7, device="cuda"), c7, cen).shape == (0, 3)          # m = 0
        cn = ops.pack_codes(empty, 7, 0, 4, bits)                                   # ncols = 0
        assert cn.nbytes == 0 and ops.packed_codebook_matmul(torch.ones(4, 7, device="cuda"), cn, cen).shape == (4, 0)
        # kdim = 1 and ncols = 1, stream and tiled
        for m in (1, 5, 40):
            x = torch.randint(-8, 9, (m, 1), device="cuda").float()
            lab = torch.randint(0, 4, (9,), device="cuda").to(torch.uint8)
            y = ops.packed_codebook_matmul(x, ops.pack_codes(lab, 1, 9, 4, bits), cen)
            assert torch.equal(y, x @ cen[lab.long()].view(1, 9))
            x = torch.randint(-8, 9, (m, 50), device="cuda").float()
            lab = torch.randint(0, 4, (50,), device="cuda").to(torch.uint8)
            y = ops.packed_codebook_matmul(x, ops.pack_codes(lab, 50, 1, 4, bits), cen, bias=bias[:1])
            assert torch.equal(y, x @ cen[lab.long()].view(50, 1) + bias[:1])
        # leading dimensions
        x = torch.randint(-8, 9, (2, 3, 7), device="cuda").float()
        lab = torch.randint(0, 4, (21,), device="cuda").to(torch.uint8)
        y = ops.packed_codebook_matmul(x, ops.pack_codes(lab, 7, 3, 4, bits), cen)
        assert y.shape == (2, 3, 3) and torch.equal(y, x @ cen[lab.long()].view(7, 3))
    codes = ops.pack_codes(torch.zeros(8, dtype=torch.uint8, device="cuda"), 4, 2, 1)
    xg = torch.ones(2, 4, device="cuda", requires_grad=True)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.packed_codebook_matmul(xg, codes, torch.ones(1, device="cuda"))
    with torch.no_grad():
        assert torch.equal(ops.packed_codebook_matmul(xg, codes, torch.ones(1, device="cuda")), torch.full((2, 2), 4.0, device="cuda"))
    with pytest.raises(ValueError):
        ops.packed_codebook_matmul(torch.ones(2, 5, device="cuda"), codes, torch.ones(1, device="cuda"))
    with pytest.raises(ValueError):
        ops.packed_codebook_matmul(torch.ones(2, 4, device="cuda"), codes, torch.ones(2, device="cuda"))
    with pytest.raises(ValueError):
        ops.packed_codebook_matmul(torch.ones(2, 4, device="cuda"), codes, torch.ones(1, device="cuda"), bias=torch.ones(3, device="cuda"))
    with pytest.raises(TypeError):
        ops.packed_codebook_matmul(torch.ones(2, 4, device="cuda"), torch.zeros(8, dtype=torch.uint8, device="cuda"), torch.ones(1, device="cuda"))


# ------------------------------------------------------------------ PackedCompressedConv2D against a float64 convolution
def _exact_conv_layer(compressed, ks, cin, cout, pad, act, rng, k):
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    lab = rng.randint(0, k, size=ks * ks * cin * cout)
    bias = rng.randint(-50, 51, size=cout).astype(np.float32)
    layer = compressed.PackedCompressedConv2D.from_codes(ks, cin, cout, pad, torch.from_numpy(lab.astype(np.uint8)).cuda(),
                                                         torch.from_numpy(cen).cuda(), torch.from_numpy(bias).cuda(), act)
    return layer, cen[lab].reshape(ks, ks, cin, cout), bias


@pytest.mark.parametrize("ks", [1, 3, 5])
@pytest.mark.parametrize("padding", ["valid", "same"])
@pytest.mark.parametrize("cin", [1, 3, 20])
def test_conv2d_bit_exact_against_a_float64_convolution(env, ks, padding, cin):
    """H != W; N * Ho * Wo <= 16 (the stream kernel) and > 16 (the tiled one); cout 1, 16, 50; K = 16 (4 bits) and 4 (2 bits)."""
    ops, compressed = env.ops, env.compressed
    pad = ks // 2 if padding == "same" else 0
    rng = np.random.RandomState(ks * 100 + cin * 3 + pad)
    for cout, k in ((1, 16), (16, 4), (50, 5)):
        for n, (ho, wo), path in ((2, (2, 3), 1), (3, (5, 4), 2)):
            hh, ww = ho + ks - 1 - 2 * pad, wo + ks - 1 - 2 * pad
            assert hh != ww
            act = torch.relu if cout != 16 else None
            layer, kernel, bias = _exact_conv_layer(compressed, ks, cin, cout, pad, act, rng, k)
            assert layer.bits == (2 if k <= 4 else 4) and layer.get_weights() == []
            assert ops.cbpk_plan(n * ho * wo, ks * ks * cin, cout, layer.bits, k, env.cus)["path"] == path
            x = rng.randint(-8, 9, size=(n, hh, ww, cin)).astype(np.float32)
            with torch.no_grad():
                got = layer(torch.from_numpy(x).cuda()).cpu().numpy()
            want = _conv_ref(x, kernel, bias, pad, act)
            assert got.shape == (n, ho, wo, cout)
            assert np.array_equal(got, want.astype(np.float32)), (cout, n)


def test_conv2d_patch_chunks_and_the_empty_batch(env, monkeypatch):
    compressed = env.compressed
    rng = np.random.RandomState(77)
    ks, cin, cout, pad = 3, 4, 16, 1
    layer, kernel, bias = _exact_conv_layer(compressed, ks, cin, cout, pad, torch.relu, rng, 16)
    x = rng.randint(-8, 9, size=(7, 6, 5, cin)).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    with torch.no_grad():
        whole = layer(xt)
    assert torch.equal(whole.cpu(), torch.from_numpy(_conv_ref(x, kernel, bias, pad, torch.relu).astype(np.float32)))
    per_image = 6 * 5 * ks * ks * cin * 4
    for per, calls in ((1, 7), (3, 3)):
        monkeypatch.setattr(compressed, "_PATCH_BYTES", per * per_image)
        seen = []
        matmul = layer._matmul
        monkeypatch.setattr(layer, "_matmul", lambda p: seen.append(p.shape[0]) or matmul(p))
        with torch.no_grad():
            got = layer(xt)
        assert seen == [per] * (7 // per) + ([7 % per] if 7 % per else []) and len(seen) == calls
        assert torch.equal(got.view(torch.int32), whole.view(torch.int32)), per
        monkeypatch.undo()
    with torch.no_grad():
        empty = layer(torch.empty(0, 6, 5, cin, device="cuda"))
    assert empty.shape == (0, 6, 5, cout) and empty.dtype == torch.float32


# ------------------------------------------------------------------ the LeNets through the Trainer
def _quantized(kind, bits, mode, n=256, seed=7):
    from neural_network_compression_amd.common import trainer as tr

    t = _trainer(kind)
    x = _inputs(kind, n, seed)
    t._prune_parameters(True)
    t.quantize(tr.LeNetDataset(x, np.zeros(n, dtype=np.int64)), mode == "density", bits, mode)   # density starts from the CDF
    return t, x


def _packed_layer_checks(env, t, cnet, x):
    """Each packed layer, fed what the decoded network feeds that layer, against a float64 product of the decoded layer."""
    compressed = env.compressed
    seen = {}
    hooks = [layer.register_forward_hook(lambda mod, inp, out, name=name: seen.__setitem__(name, inp[0].detach().clone()))
             for name, layer in t.neural_network.get_config().items()]
    with torch.no_grad():
        t.neural_network(x)
    for h in hooks:
        h.remove()
    checked = 0
    for name, layer in cnet.get_config().items():
        if not isinstance(layer, compressed._PackedCodebookLayer):
            continue
        inp = seen[name]
        with torch.no_grad():
            y = layer(inp).cpu().numpy()
        orig = t.neural_network.get_config()[name]
        w_dec, b = orig.kernel.detach().cpu().numpy(), orig.bias.detach().cpu().numpy()
        if isinstance(layer, compressed.PackedCompressedConv2D):
            ks = w_dec.shape[0]
            rows = compressed.keras_rows_for_unfold(ks, ks, w_dec.shape[2])
            p = compressed.conv_patches(inp.cpu().double(), ks, layer.pad).numpy()
            xin, w = p.reshape(-1, p.shape[-1]), w_dec.reshape(-1, w_dec.shape[-1])[rows]
            y = y.reshape(-1, y.shape[-1])
        else:
            xin, w = inp.cpu().numpy(), w_dec
        x64, w64 = xin.astype(np.float64), w.astype(np.float64)
        pre = x64 @ w64 + b
        ref = np.maximum(pre, 0) if orig.activation is torch.relu else pre
        err = np.abs(y.astype(np.float64) - ref)
        bound = 2.0 * xin.shape[-1] * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64) + np.abs(b)) + 1e-30
        assert np.all(err <= bound), (name, float((err / bound).max()))
        checked += 1
    return checked


def _make_exact(t):
    """The fitted centres replaced by -1, 0 and 1 (0 for each tensor's most frequent index): with sparse binary inputs every
    partial sum of the network is a small integer.  A bias too short to be quantized stays raw: it is rounded to integers."""
    for layer, models in t.quantized_models_by_layer.items():
        if len(models) < 2 or models[1] is None:
            with torch.no_grad():
                layer.bias.copy_(torch.round(layer.bias * 16))
        for mdl in models:
            if mdl is None:
                continue
            k = mdl.cluster_centers_.size
            cen = np.array([1.0 if j % 2 == 0 else -1.0 for j in range(k)], dtype=np.float32)
            counts = np.bincount(mdl.labels_compact_.cpu().numpy().astype(np.int64).ravel(), minlength=k)
            cen[int(counts.argmax())] = 0.0
            mdl.cluster_centers_ = cen.reshape(mdl.cluster_centers_.shape)


@pytest.mark.parametrize("kind,bits,mode,want_k,want_bits", [("lenet300", 4, "linear", 16, 4), ("lenet300", 2, "linear", 4, 2),
                                                             ("lenet300", 2, "density", 5, 4), ("lenet5", 4, "linear", 16, 4)])
def test_lenets_through_the_trainer(env, kind, bits, mode, want_k, want_bits):
    compressed = env.compressed
    t, x = _quantized(kind, bits, mode)
    ks = [m.cluster_centers_.size for ms in t.quantized_models_by_layer.values() for m in ms if m is not None]
    assert ks and max(ks) == want_k
    xt = torch.from_numpy(x).cuda()
    cnet = t.compressed_network(packed=True)
    quantized = [cnet.get_config()[name] for name, layer in t.neural_network.get_config().items()
                 if (t.quantized_models_by_layer.get(layer) or [None])[0] is not None]
    assert len(quantized) == (3 if kind == "lenet300" else 4) and all(isinstance(l, compressed._PackedCodebookLayer) for l in quantized)      # every K <= 16: all packed
    assert all(l.bits == (2 if l.k <= 4 else 4) for l in quantized) and max(l.bits for l in quantized) == want_bits
    for l in quantized:
        assert l.nbytes() == l.kdim * packed_ref.row_bytes(l.ncols, l.bits) + 4 * l.k + 4 * l.ncols
    assert _packed_layer_checks(env, t, cnet, xt) == len(quantized) >= 2
    # dyadic centres and integer inputs: the packed network is the byte-form network bit for bit
    _make_exact(t)
    byte_net, packed_net = t.compressed_network(), t.compressed_network(packed=True)
    rng = np.random.RandomState(31)
    xe = (rng.rand(*x[:64].shape) < 0.1).astype(np.float32)
    if kind == "lenet300":                                   # the precondition, layer by layer, on the decoded byte-form layers
        h = xe.astype(np.float64)
        for layer in byte_net.get_config().values():
            w = env.ops.gather(layer.centers, layer.labels).cpu().numpy().astype(np.float64).reshape(layer.kdim, layer.ncols)
            b = layer.bias.cpu().numpy().astype(np.float64)
            assert_exact(h, w, b)
            h = h @ w + b
            h = np.maximum(h, 0) if layer.activation is torch.relu else h
    xet = torch.from_numpy(xe).cuda()
    with torch.no_grad():
        got, want = packed_net(xet), byte_net(xet)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert float(want.abs().max()) < 2.0 ** 24 and torch.equal(want, want.round())      # integers throughout: nothing was rounded
    if kind == "lenet300":
        assert np.array_equal(got.cpu().numpy(), h.astype(np.float32))


def test_footprint_and_auto_selection_on_lenet_300_100(env):
    compressed = env.compressed
    t, _ = _quantized("lenet300", 4, "linear", n=64, seed=3)
    auto, byte_net = t.compressed_network(packed="auto"), t.compressed_network()
    want_total = 0
    for name, layer in t.neural_network.get_config().items():
        w, b = layer.get_weights()
        k = t.quantized_models_by_layer[layer][0].cluster_centers_.size
        assert k <= 16
        kdim, ncols = w.shape
        byte_bytes, packed_bytes = kdim * ncols, kdim * packed_ref.row_bytes(ncols, 2 if k <= 4 else 4)
        c = auto.get_config()[name]
        want_cls = compressed.PackedCompressedDense if packed_bytes < byte_bytes else compressed.CompressedDense
        assert type(c) is want_cls, (name, type(c))
        assert compressed.compressed_nbytes(c) == min(byte_bytes, packed_bytes) + 4 * k + 4 * ncols
        want_total += min(byte_bytes, packed_bytes) + 4 * k + 4 * ncols
    assert type(auto.get_config()["out"]) is compressed.CompressedDense          # 100 x 10: 16-byte rows against 10-byte ones
    assert compressed.compressed_nbytes(auto) == want_total < compressed.compressed_nbytes(byte_net)
    assert compressed.compressed_nbytes(auto) < 0.56 * compressed.compressed_nbytes(byte_net)
    forced = t.compressed_network(packed=True)
    assert all(isinstance(l, compressed.PackedCompressedDense) for l in forced.get_config().values())


def _codes_model(centers, labels):
    return SimpleNamespace(cluster_centers_=np.asarray(centers, dtype=np.float32).reshape(-1, 1), labels_compact_=labels)


class _ThreeDense(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from neural_network_compression_amd.neural_networks.layers import Dense

        self.wide, self.pruned, self.narrow = Dense(64, 256, activation=torch.relu), Dense(256, 512, activation=torch.relu), Dense(512, 10)

    def get_config(self):
        return {"wide": self.wide, "pruned": self.pruned, "narrow": self.narrow}

    def forward(self, x):
        return self.narrow(self.pruned(self.wide(x)))


def test_each_form_wins_one_layer_under_the_three_way_rule(env):
    """A wide dense 4-bit layer (packed: half the bytes), a 99 %-pruned one (bitmap-sparse: ~2 bits a weight against 4) and a
    10-column one (byte form: 10-byte rows against padded 16-byte ones); then the forced and the excluded combinations."""
    compressed, ops = env.compressed, env.ops
    rng = np.random.RandomState(12)
    net = _ThreeDense().cuda()
    cen = (np.arange(16) - 8).astype(np.float32) / 8.0
    models = {}
    for name, layer in net.get_config().items():
        n = layer.kernel.numel()
        lab = rng.randint(0, 16, size=n)
        if name == "pruned":
            lab = np.where(rng.rand(n) < 0.99, 8, lab)
        bl = rng.randint(0, 16, size=layer.bias.numel())
        kt, bt = torch.from_numpy(lab.astype(np.uint8)).cuda(), torch.from_numpy(bl.astype(np.uint8)).cuda()
        layer.set_weights([torch.from_numpy(cen[lab]).cuda().view(layer.kernel.shape), torch.from_numpy(cen[bl]).cuda()])
        models[layer] = [_codes_model(cen, kt), _codes_model(cen, bt)]
    x = torch.from_numpy((rng.rand(9, 64) < 0.2).astype(np.float32)).cuda()
    with torch.no_grad():
        want = compressed.compress_network(net, models)(x)

    def forms(**kw):
        cnet = compressed.compress_network(net, models, **kw)
        with torch.no_grad():
            assert torch.equal(cnet(x).view(torch.int32), want.view(torch.int32)), kw      # exact data: every form, the same bits
        return [type(l).__name__ for l in cnet.get_config().values()], cnet

    B, S, P = "CompressedDense", "SparseCompressedDense", "PackedCompressedDense"
    got, cnet = forms(sparse="auto", packed="auto")
    assert got == [P, S, B]
    assert cnet.wide.nbytes() == 64 * 128 + 4 * 16 + 4 * 256 and cnet.narrow.nbytes() == 512 * 10 + 4 * 16 + 4 * 10
    assert cnet.pruned.nbytes() < 256 * 256
    assert forms(packed="auto")[0] == [P, P, B]
    assert forms(packed=True)[0] == [P, P, P]
    assert forms(sparse="auto", packed=True)[0] == [P, S, P]          # the byte form is excluded for K <= 16 ...
    assert forms(sparse=True, packed="auto")[0] == [P, S, P]          # ... and by sparse=True: 8192 bytes of padded rows beat ~13 K sparse
    assert forms(sparse="auto")[0] == [B, S, B] and forms()[0] == [B, B, B]
    with pytest.raises(ValueError):
        compressed.compress_network(net, models, sparse=True, packed=True)
    with pytest.raises(ValueError, match="inference only"):
        compressed.compress_network(net, models, trainable=True, packed=True)
    assert ops.pack_codes(models[net.wide][0].labels_compact_, 64, 256, 16).nbytes == 64 * 128


def test_load_network_packs_what_the_stored_file_holds(env, tmp_path):
    compressed = env.compressed
    for kind in ("lenet300", "lenet5"):
        t, x = _quantized(kind, 4, "linear", n=64, seed=9)
        xt = torch.from_numpy(x).cuda()
        want_net = t.compressed_network(packed="auto")
        with torch.no_grad():
            want = want_net(xt)
        t.store_report(str(tmp_path / kind))
        got_net = compressed.load_network(str(tmp_path / kind / "weights.nnc"), t.neural_network, packed="auto")
        assert [type(l) for l in got_net.get_config().values()] == [type(l) for l in want_net.get_config().values()]
        assert any(isinstance(l, compressed._PackedCodebookLayer) for l in got_net.get_config().values())
        for a, b in zip(got_net.get_config().values(), want_net.get_config().values()):
            if isinstance(a, compressed._PackedCodebookLayer):
                assert torch.equal(a.packed, b.packed) and torch.equal(a.centers.view(torch.int32), b.centers.view(torch.int32))
        with torch.no_grad():
            got = got_net(xt)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), kind
        assert compressed.compressed_nbytes(got_net) == compressed.compressed_nbytes(want_net)


def test_seventeen_centres_stay_in_the_byte_form(env):
    """A 4-bit density fit has K = 17: pack_codes raises, packed=True and "auto" leave the layer a CompressedDense with today's bits."""
    compressed, ops = env.compressed, env.ops
    t, x = _quantized("lenet300", 4, "density", n=64, seed=5)
    by_layer = t.quantized_models_by_layer
    ks = {name: by_layer[layer][0].cluster_centers_.size for name, layer in t.neural_network.get_config().items()}
    assert max(ks.values()) == 17
    name17 = [n for n, k in ks.items() if k == 17][0]
    wm = by_layer[t.neural_network.get_config()[name17]][0]
    kdim, ncols = t.neural_network.get_config()[name17].kernel.shape
    with pytest.raises(ValueError, match="16"):
        ops.pack_codes(wm.labels_compact_, kdim, ncols, 17)
    with pytest.raises(ValueError):
        compressed.PackedCompressedDense.from_dense(t.neural_network.get_config()[name17], wm)
    xt = torch.from_numpy(x).cuda()
    base = t.compressed_network()
    with torch.no_grad():
        want = base(xt)
    for packed in (True, "auto"):
        cnet = t.compressed_network(packed=packed)
        layer = cnet.get_config()[name17]
        assert type(layer) is compressed.CompressedDense
        assert torch.equal(layer.labels, base.get_config()[name17].labels)
        seen = {}
        h = base.get_config()[name17].register_forward_hook(lambda mod, inp, out: seen.__setitem__("x", inp[0].detach().clone()))
        with torch.no_grad():
            base(xt)
        h.remove()
        with torch.no_grad():
            assert torch.equal(layer(seen["x"]).view(torch.int32), base.get_config()[name17](seen["x"]).view(torch.int32))
        if all(k > 16 for k in ks.values()):
            with torch.no_grad():
                assert torch.equal(cnet(xt).view(torch.int32), want.view(torch.int32))
    with pytest.raises(ValueError, match="inference only"):
        t.compressed_network(trainable=True, packed=True)
    with pytest.raises(ValueError):
        t.compressed_network(sparse=True, packed=True)
