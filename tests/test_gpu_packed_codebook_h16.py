"""The 2- / 4-bit packed codebook matmul on bf16 / fp16 activations (nnc_cbpk_h16, csrc/nnc_cbpk_h16.hip),
through the raw C ABI with buffers the test owns, through ops.packed_codebook_matmul, through the packed inference layers built with
half_inputs=True and through compress_network / load_network(packed=..., packed_half_inputs=True) (run with -m gpu).

What it is held to needs no tolerance.  At every m the result is ops.grouped_packed_codebook_matmul with one group bit for bit; above
16 rows of x it is ops.codebook_matmul on the unpacked labels bit for bit; up to 16 rows the float32 result is
ops.packed_codebook_matmul on the widened x and the centres rounded to the dtype and widened, bit for bit; a half result is the
float32 one rounded once.  Every raw call writes into sentinel-framed y and workspace and is repeated for the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import h16_ref  # noqa: E402
from tests.helpers import packed_h16_ref as pref  # noqa: E402
from tests.helpers import packed_ref  # noqa: E402
from tests.helpers.cbmm_ref import matmul64, relu_like_torch  # noqa: E402
from tests.helpers.h16_ref import DTYPES, round_to  # noqa: E402

SENT16 = 0x7FA5              # as bf16 and as fp16 a NaN whose payload neither the inputs nor the kernels' own NaNs carry
SENT32 = 0x7FA57FA5
WS_PAD = 64

# packed_ref's cases (every stream plan, split and direct; the tiled ones become the MFMA tile) and the MFMA rows of the backward list
FORWARD = list(packed_ref.PACKED_REGIME_CASES) + [
    dict(m=c[0][1], kdim=c[0][2], ncols=c[0][3], bits=c[0][4], k=c[0][5], x_view=c[1], bias=i % 2 == 0, bias_view=False) for i, c in enumerate(pref.MFMA_FORWARD)]


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, ops

    L = _native.load()
    _, cus = ops.device_info()
    assert cus >= 1
    return L, ops, cus


def _tdt(dtype):
    return h16_ref.torch_dtype(dtype)


def _bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64, 2: torch.int16}[t.element_size()])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same_or_both_nan(a, b):
    """the same bits, or a NaN on both sides (a NaN's payload and sign are not part of the contract)"""
    return a.dtype == b.dtype and a.shape == b.shape and bool(((_bits(a) == _bits(b)) | (torch.isnan(a) & torch.isnan(b))).all())


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _half(host, dtype, view=False):
    """host values -> a device tensor of the dtype that ends directly in front of NaN bit patterns; ``view``: it starts one element
    into its buffer (aligned to the element size and no further)."""
    t = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).to(_tdt(dtype))
    off = 1 if view else 0
    buf = torch.full((off + t.numel() + 64,), -1, dtype=torch.int16, device="cuda")
    x = buf[off: off + t.numel()].view(_tdt(dtype))
    x.copy_(t.reshape(-1))
    return x.view(t.shape)


def _codes(env, lab, bits, k):
    """the packed form of lab (kdim, ncols) at the very end of its tensor (256 bytes of 0xFF in front keep the alignment)"""
    _, ops, _ = env
    kdim, ncols = lab.shape
    codes = ops.pack_codes(_cuda(lab.astype(np.uint8).ravel()), kdim, ncols, k, bits)
    big = torch.full((256 + codes.nbytes,), 255, dtype=torch.uint8, device="cuda")
    big[256:] = codes.packed
    return ops.PackedCodes(big[256:], kdim, ncols, bits, k)


def _call(env, x, dtype, m, codes, centers, bias, relu, half_out):
    """nnc_cbpk_h16 into sentinel-framed y and workspace (exactly the queried size); checks the frames; returns y (m, ncols)."""
    L, ops, _ = env
    kdim, ncols = codes.kdim, codes.ncols
    ws_bytes = int(L.nnc_cbpk_h16_workspace_bytes(m, kdim, ncols, codes.bits))
    assert ws_bytes % 4 == 0
    mn = m * ncols
    units, pad = (mn, 37) if half_out else (2 * mn, 38)
    ybuf = torch.full((units + 2 * pad,), SENT16, dtype=torch.int16, device="cuda")
    wsbuf = torch.full((ws_bytes // 4 + 2 * WS_PAD,), SENT32, dtype=torch.int32, device="cuda")
    y = ybuf[pad: pad + units]
    dt = h16_ref.DT_CODE[dtype]
    ops.nat.check(L.nnc_cbpk_h16(x.data_ptr(), dt, m, kdim, codes.packed.data_ptr(), codes.nbytes, codes.bits, ncols, centers.data_ptr(), centers.numel(),
                                 None if bias is None else bias.data_ptr(), int(relu), y.data_ptr(), dt if half_out else 0,
                                 wsbuf[WS_PAD:].data_ptr() if ws_bytes else None, ws_bytes, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((ybuf[:pad] == SENT16).all()) and bool((ybuf[pad + units:] == SENT16).all()), "a store outside y"
    assert bool((wsbuf[:WS_PAD] == SENT32).all()) and bool((wsbuf[WS_PAD + ws_bytes // 4:] == SENT32).all()), "a store outside the workspace"
    if half_out:
        assert not bool((y == SENT16).any()), "an output left unwritten"
        return y.clone().view(_tdt(dtype)).view(m, ncols)
    assert not bool((y.view(torch.int32) == SENT32).any()), "an output left unwritten"
    return y.clone().view(torch.float32).view(m, ncols)


def test_the_forward_cases_hit_every_path_at_this_device(env):
    _, ops, cus = env
    hit = set()
    for c in FORWARD:
        p = ops.cbpk_h16_plan(torch.bfloat16, c["m"], c["kdim"], c["ncols"], c["bits"], c["k"], cus)
        assert p["path"] == (h16_ref.PATH_MFMA if c["m"] > 16 else h16_ref.PATH_STREAM)
        hit.add((p["path"], c["bits"], p["splits"] > 1))
    assert {(path, b, s) for path in (h16_ref.PATH_STREAM, h16_ref.PATH_MFMA) for b in (2, 4) for s in (False, True)} <= hit


@pytest.fixture(scope="module")
def case_data(env):
    """Per case, made once and left unchanged: the labels (some beyond K where K < 2^bits), their packed form, float and exact data."""
    out = []
    for ci, c in enumerate(FORWARD):
        rng = np.random.RandomState(9000 + ci)
        k, bits = c["k"], c["bits"]
        lab = rng.randint(0, k, size=(c["kdim"], c["ncols"]))
        if ci % 3 == 0 and k < (1 << bits) and lab.size:
            lab[rng.rand(*lab.shape) < 0.1] = (1 << bits) - 1
        out.append(dict(lab=lab, codes=_codes(env, lab, bits, k), cf=rng.standard_normal(k).astype(np.float32),
                        cen=(rng.randint(-16, 17, size=k) / 4.0).astype(np.float32),
                        xf=rng.standard_normal((c["m"], c["kdim"])).astype(np.float32), bf=rng.standard_normal(c["ncols"]).astype(np.float32),
                        x=rng.randint(-8, 9, size=(c["m"], c["kdim"])).astype(np.float32),
                        bias=rng.randint(-50, 51, size=c["ncols"]).astype(np.float32)))
    return out


def _check_against_its_definition(env, c, dtype, codes, x_t, cen_t, bias_t, relu, same=_same):
    """One call of each output type against the three parts of the contract; returns the two results."""
    _, ops, _ = env
    tdt, m = _tdt(dtype), c["m"]
    got32 = _call(env, x_t, dtype, m, codes, cen_t, bias_t, relu, False)
    got16 = _call(env, x_t, dtype, m, codes, cen_t, bias_t, relu, True)
    group_rows = max(32, 32 * -(-codes.kdim // 32))
    cg = cen_t.view(1, -1)
    assert same(got32, ops.grouped_packed_codebook_matmul(x_t, codes, cg, group_rows, bias=bias_t, relu=relu, out_dtype=torch.float32)), (c, dtype)
    assert same(got16, ops.grouped_packed_codebook_matmul(x_t, codes, cg, group_rows, bias=bias_t, relu=relu)), (c, dtype)
    if m > 16:
        dense = codes.to_dense()
        assert same(got32, ops.codebook_matmul(x_t, dense, cen_t, codes.kdim, codes.ncols, bias=bias_t, relu=relu, out_dtype=torch.float32)), (c, dtype)
        assert same(got16, ops.codebook_matmul(x_t, dense, cen_t, codes.kdim, codes.ncols, bias=bias_t, relu=relu)), (c, dtype)
    else:
        assert same(got32, ops.packed_codebook_matmul(x_t.float(), codes, cen_t.to(tdt).float(), bias=bias_t, relu=relu)), (c, dtype)
    assert same(got16, got32.to(tdt))                                  # the half output is one rounding of the float32 value
    return got32, got16


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci", range(len(FORWARD)), ids=[f"{i}-" + packed_ref.case_id(c) for i, c in enumerate(FORWARD)])
def test_case(env, case_data, ci, dtype):
    _, ops, _ = env
    c, d = FORWARD[ci], case_data[ci]
    m, kdim, k = c["m"], c["kdim"], c["k"]
    tdt, codes, lab = _tdt(dtype), d["codes"], d["lab"]
    assert torch.equal(codes.to_dense().cpu().reshape(lab.shape), torch.from_numpy(lab.astype(np.uint8)))
    xf_t, cf_t = _half(d["xf"], dtype, c["x_view"]), _cuda(d["cf"])
    for bias_t, relu in ((_cuda(d["bf"]) if c["bias"] else None, True), (None, False), (_cuda(d["bf"]), False)):
        got32, got16 = _check_against_its_definition(env, c, dtype, codes, xf_t, cf_t, bias_t, relu)
        assert bool(torch.isfinite(got32).all())
        # the same bits a second time, and through ops
        assert _same(got32, _call(env, xf_t, dtype, m, codes, cf_t, bias_t, relu, False))
        assert _same(got16, _call(env, xf_t, dtype, m, codes, cf_t, bias_t, relu, True))
        assert _same(got32, ops.packed_codebook_matmul(xf_t, codes, cf_t, bias=bias_t, relu=relu, out_dtype=torch.float32))
        assert _same(got16, ops.packed_codebook_matmul(xf_t, codes, cf_t, bias=bias_t, relu=relu))
    # a NaN in x is kept through ReLU
    xn = round_to(d["xf"], dtype)
    xn[m - 1, kdim - 1] = np.nan
    n32, n16 = _check_against_its_definition(env, c, dtype, codes, _half(xn, dtype, c["x_view"]), cf_t, None, True, same=_same_or_both_nan)
    assert bool(torch.isnan(n32[m - 1]).all()) and bool(torch.isnan(n16[m - 1]).all())
    # exact data: the float64 product with the decoded W (a label >= K reads 0) bit for bit, in float32 and (rounded once) in half
    w = np.append(d["cen"], np.float32(0.0))[np.minimum(lab, k)]
    bias = d["bias"] if c["bias"] else None
    want = matmul64(d["x"], w, bias)
    assert 4 * (np.abs(d["x"].astype(np.float64)) @ np.abs(w.astype(np.float64))).max(initial=0.0) + 200 < 2.0 ** 22
    for relu in (False, True):
        ref = (relu_like_torch(want) if relu else want).astype(np.float32)
        e32, e16 = _check_against_its_definition(env, c, dtype, codes, _half(d["x"], dtype, c["x_view"]), _cuda(d["cen"]),
                                                 None if bias is None else _cuda(bias), relu)
        assert np.array_equal(e32.cpu().numpy(), ref), (c, dtype)
        assert np.array_equal(e16.float().cpu().numpy(), round_to(ref, dtype)), (c, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kdim,ncols,bits,k", [(33, 50, 4, 16), (64, 129, 2, 4), (300, 129, 4, 5), (1001, 200, 2, 3)])
def test_m16_and_m17_rows_agree(env, dtype, kdim, ncols, bits, k):
    """The first 16 rows through the stream kernel (m = 16) and through the MFMA tile (m = 17), on the same exact data: the same bits"""
    rng = np.random.RandomState(kdim)
    lab = rng.randint(0, k, size=(kdim, ncols))
    x = rng.randint(-8, 9, size=(17, kdim)).astype(np.float32)
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    bias = rng.randint(-50, 51, size=ncols).astype(np.float32)
    codes = _codes(env, lab, bits, k)
    x_t, cen_t, bias_t = _half(x, dtype), _cuda(cen), _cuda(bias)
    for half_out in (False, True):
        y16 = _call(env, x_t[:16], dtype, 16, codes, cen_t, bias_t, True, half_out)
        y17 = _call(env, x_t, dtype, 17, codes, cen_t, bias_t, True, half_out)
        assert _same(y16, y17[:16]), half_out


def test_degenerate_shapes_and_python_errors(env):
    """m = 0 and ncols = 0 write nothing; kdim = 0 writes the bias (ReLU applied), in float32 and in half; the dtype rules of ops"""
    _, ops, _ = env
    cen_t = torch.ones(4, device="cuda")
    bias = np.array([-1.5, 2.25, 0.0, 1000.0, -3.0], dtype=np.float32)
    bias_t = _cuda(bias)
    empty = ops.pack_codes(torch.zeros(0, dtype=torch.uint8, device="cuda"), 0, 5, 4)
    codes = ops.pack_codes(torch.zeros(7 * 5, dtype=torch.uint8, device="cuda"), 7, 5, 4)
    for dtype in DTYPES:
        for m in (3, 20):
            x_t = torch.zeros((m, 0), dtype=_tdt(dtype), device="cuda")
            for half_out in (False, True):
                y = _call(env, x_t, dtype, m, empty, cen_t, bias_t, True, half_out)
                assert np.array_equal(y.float().cpu().numpy(), np.tile(np.maximum(bias, 0), (m, 1)))
        assert ops.packed_codebook_matmul(torch.zeros((0, 7), dtype=_tdt(dtype), device="cuda"), codes, cen_t).shape == (0, 5)
        x_t = torch.zeros((2, 7), dtype=_tdt(dtype), device="cuda")
        assert ops.packed_codebook_matmul(x_t, codes, cen_t).dtype == _tdt(dtype)
        assert ops.packed_codebook_matmul(x_t, codes, cen_t, out_dtype=torch.float32).dtype == torch.float32
        other = torch.float16 if dtype == "bf16" else torch.bfloat16
        for kw in (dict(out_dtype=other), dict(out_dtype=torch.float64), dict(bias=bias_t.to(_tdt(dtype))), dict(centers=cen_t.to(_tdt(dtype)))):
            args = dict(centers=cen_t, bias=bias_t, out_dtype=None)
            args.update(kw)
            with pytest.raises(TypeError):
                ops.packed_codebook_matmul(x_t, codes, args["centers"], bias=args["bias"], out_dtype=args["out_dtype"])
        with pytest.raises(RuntimeError, match="inference only"):
            ops.packed_codebook_matmul(x_t.clone().requires_grad_(), codes, cen_t)
    with pytest.raises(TypeError):
        ops.packed_codebook_matmul(torch.zeros((2, 7), dtype=torch.float64, device="cuda"), codes, cen_t)
    with pytest.raises(TypeError):
        ops.packed_codebook_matmul(torch.zeros((2, 7), device="cuda"), codes, cen_t, out_dtype=torch.bfloat16)
    assert ops.packed_codebook_matmul(torch.zeros((2, 7), device="cuda"), codes, cen_t, out_dtype=torch.float32).dtype == torch.float32


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_makes_no_host_read(env, dtype):
    _, ops, _ = env
    rng = np.random.RandomState(3)
    codes = _codes(env, rng.randint(0, 16, size=(90, 150)), 4, 16)
    cen_t, bias_t = _cuda(rng.standard_normal(16).astype(np.float32)), _cuda(rng.standard_normal(150).astype(np.float32))
    xs = [_half(rng.standard_normal((m, 90)), dtype) for m in (5, 40)]
    for x in xs:
        ops.packed_codebook_matmul(x, codes, cen_t, bias=bias_t, relu=True)   # (warm: allocations, the library load)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for x in xs:
            ops.packed_codebook_matmul(x, codes, cen_t, bias=bias_t, relu=True)
            ops.packed_codebook_matmul(x, codes, cen_t, out_dtype=torch.float32)
    finally:
        torch.cuda.set_sync_debug_mode(0)


# ------------------------------------------------------------------ layers
def _layer_data(rng, kdim, ncols, k):
    lab = rng.randint(0, k, size=kdim * ncols).astype(np.uint8)
    return _cuda(lab), _cuda(rng.standard_normal(k).astype(np.float32)), _cuda(rng.standard_normal(ncols).astype(np.float32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_layers_with_half_inputs_equal_the_op_and_chain_in_half(env, dtype):
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    tdt = _tdt(dtype)
    rng = np.random.RandomState(11)
    l1 = compressed.PackedCompressedDense.from_codes(64, 48, *_layer_data(rng, 64, 48, 9), torch.relu, half_inputs=True)
    l2 = compressed.PackedCompressedDense.from_codes(48, 10, *_layer_data(rng, 48, 10, 4), None, None, True)
    plain = compressed.PackedCompressedDense(l1.codes, l1.centers, l1.bias, torch.relu)
    assert l1.half_inputs and l2.half_inputs and not plain.half_inputs and (l1.bits, l2.bits) == (4, 2)
    for m in (3, 40):
        xf = torch.from_numpy(rng.standard_normal((m, 64)).astype(np.float32)).cuda()
        x = xf.to(tdt)
        with torch.no_grad():
            h = l1(x)
            y = l2(h)
            assert _same(l1(xf), plain(xf))                            # a float32 input takes the float32 path, option or not
            with pytest.raises(TypeError, match="float32 activations"):
                plain(x)
        assert h.dtype == tdt and y.dtype == tdt
        assert _same(h, ops.packed_codebook_matmul(x, l1.codes, l1.centers, bias=l1.bias, relu=True))
        assert _same(y, ops.packed_codebook_matmul(h, l2.codes, l2.centers, bias=l2.bias))
        with pytest.raises(RuntimeError, match="inference only"):
            l1(x.clone().requires_grad_())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ks,cin,cout,pad", [(3, 4, 16, 1), (5, 1, 6, 0)])
def test_conv2d_with_half_inputs_equals_the_op_and_chunks_by_the_element_size(env, dtype, ks, cin, cout, pad, monkeypatch):
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    tdt = _tdt(dtype)
    rng = np.random.RandomState(12)
    lab_t, cen_t, bias_t = _layer_data(rng, ks * ks * cin, cout, 16)
    layer = compressed.PackedCompressedConv2D.from_codes(ks, cin, cout, pad, lab_t, cen_t, bias_t, torch.relu, half_inputs=True)
    plain = compressed.PackedCompressedConv2D.from_codes(ks, cin, cout, pad, lab_t, cen_t, bias_t, torch.relu)
    x = torch.from_numpy(rng.standard_normal((7, 8, 7, cin)).astype(np.float32)).cuda().to(tdt)
    with torch.no_grad():
        whole = layer(x)
        with pytest.raises(TypeError, match="float32 activations"):
            plain(x)
    ho, wo = 8 + 2 * pad - ks + 1, 7 + 2 * pad - ks + 1
    assert whole.dtype == tdt and whole.shape == (7, ho, wo, cout)
    patches = compressed.conv_patches(x, ks, pad).contiguous()
    assert _same(whole.reshape(-1, cout), ops.packed_codebook_matmul(patches, layer.codes, layer.centers, bias=layer.bias, relu=True).reshape(-1, cout))
    per_image = ho * wo * ks * ks * cin * 2           # 2 bytes an element
    for per, calls in ((1, 7), (3, 3)):
        monkeypatch.setattr(compressed, "_PATCH_BYTES", per * per_image)
        seen = []
        matmul = layer._matmul
        monkeypatch.setattr(layer, "_matmul", lambda p: seen.append(p.shape[0]) or matmul(p))
        with torch.no_grad():
            got = layer(x)
        assert seen == [per] * (7 // per) + ([7 % per] if 7 % per else []) and len(seen) == calls
        assert _same(got, whole), per
        monkeypatch.undo()
    with torch.no_grad():
        empty = layer(torch.empty(0, 8, 7, cin, dtype=tdt, device="cuda"))
    assert empty.shape == (0, ho, wo, cout) and empty.dtype == tdt


@pytest.mark.parametrize("kind", ["lenet300", "lenet5"])
def test_compress_network_and_load_network_with_packed_half_inputs(env, kind, tmp_path):
    """packed="auto": what it picks does not change with the option; the packed layers take half inputs and chain in half, every layer
    equal to its op on what the layer before gave; the stored file loads into the same network"""
    from neural_network_compression_amd import compressed
    from neural_network_compression_amd.common import trainer as tr
    from tests.test_gpu_codebook_matmul import _inputs, _trainer

    _, ops, _ = env
    t = _trainer(kind)
    x = _inputs(kind, 40, 9)
    t._prune_parameters(True)
    t.quantize(tr.LeNetDataset(x, np.zeros(40, dtype=np.int64)), False, 4, "linear")
    plain = t.compressed_network(packed="auto")
    half = t.compressed_network(packed="auto", packed_half_inputs=True)
    t.store_report(str(tmp_path))
    loaded = compressed.load_network(str(tmp_path / "weights.nnc"), t.neural_network, packed="auto", packed_half_inputs=True)
    assert [type(l) for l in plain.get_config().values()] == [type(l) for l in half.get_config().values()] == [type(l) for l in loaded.get_config().values()]
    assert compressed.compressed_nbytes(plain) == compressed.compressed_nbytes(half)
    packed = [l for l in half.get_config().values() if isinstance(l, compressed._PackedCodebookLayer)]
    assert packed and all(l.half_inputs for l in packed) and all(l.half_inputs for l in loaded.get_config().values() if isinstance(l, compressed._PackedCodebookLayer))
    assert not any(l.half_inputs for l in plain.get_config().values() if isinstance(l, compressed._PackedCodebookLayer))
    xt = torch.from_numpy(x).cuda()
    for tdt in (torch.bfloat16, torch.float16):
        seen = []
        hooks = [l.register_forward_hook(lambda mod, inp, out: seen.append((mod, inp[0].detach(), out.detach()))) for l in half.get_config().values()]
        with torch.no_grad():
            y = half(xt.to(tdt))
            with pytest.raises(TypeError, match="float32 activations"):
                plain(xt.to(tdt))
            assert _same(y, loaded(xt.to(tdt)))
        for h in hooks:
            h.remove()
        assert y.dtype == tdt
        for mod, inp, out in seen:
            assert inp.dtype == tdt and out.dtype == tdt
            if isinstance(mod, compressed.PackedCompressedDense):
                assert _same(out, ops.packed_codebook_matmul(inp, mod.codes, mod.centers, bias=mod.bias, relu=mod._fused_relu))
    with torch.no_grad():
        assert _same(half(xt), plain(xt))                               # a float32 input takes the float32 path, option or not
