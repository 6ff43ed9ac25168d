"""The bitmap-sparse codebook matmul on bf16 / fp16 activations (nnc_cbsp_h16, csrc/nnc_cbsp_h16.hip),
through the raw C ABI with buffers the test owns, through ops.sparse_codebook_matmul and through the layers (run with -m gpu).

What it is held to needs no tolerance.  Above 16 rows of x (k_cbsp_mfma) the result is ops.codebook_matmul on the unpacked labels bit
for bit, non-finite inputs included; up to 16 rows (k_cbsp_stream on half x) the float32 result is the float32 sparse product of the
widened x and the rounded centres bit for bit, and a half result is that value rounded once.  On exact data (integer x, quarter-
integer centres, an integer bias: every partial sum is exact in float32 in any order) both equal the float64 product with the
decoded W.  Every raw call writes into sentinel-framed y and workspace slices (2-byte granularity for a half y), reads x directly in
front of NaN bit patterns and the symbols at the very end of their tensor, and is repeated for the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import h16_ref, sparse_h16_ref  # noqa: E402
from tests.helpers.cbmm_ref import matmul64, relu_like_torch  # noqa: E402
from tests.helpers.h16_ref import DTYPES, round_to  # noqa: E402
from tests.helpers.sparse_h16_ref import CASES  # noqa: E402
from tests.helpers.sparse_ref import labels_at_density  # noqa: E402

SENT16 = 0x7FA5              # as bf16 and as fp16 a NaN whose payload neither the inputs nor the kernels' own NaNs carry
SENT32 = 0x7FA57FA5          # two of them: a float32 NaN of the same kind
WS_PAD = 64                  # sentinel words on each side of the workspace


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
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    """the same dtype, shape and bits"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _same_or_both_nan(a, b):
    """the same bits, or a NaN on both sides (torch's conversion to a half type gives the canonical NaN, a kernel's need not)"""
    return a.dtype == b.dtype and a.shape == b.shape and bool(((_bits(a) == _bits(b)) | (torch.isnan(a) & torch.isnan(b))).all())


def _dev_x(host, tdtype, view):
    """host float32 values (exact in ``tdtype``, or rounded by torch) -> a device tensor that ends directly in front of NaN bit
    patterns (0xFFFF units); ``view``: it starts one element into its buffer (aligned to the element size and no further)."""
    t = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).to(tdtype)
    off = 1 if view else 0
    buf = torch.full((off + t.numel() + 64,), -1, dtype=torch.int16, device="cuda")
    x = buf[off: off + t.numel()].view(tdtype)
    x.copy_(t.reshape(-1))
    assert bool(torch.isnan(buf[off + t.numel():].view(tdtype).float()).all())
    return x.view(t.shape)


def _dev_labels(lab, lb):
    host = np.ascontiguousarray(lab, dtype=np.uint8 if lb == 1 else np.uint16).ravel()
    return torch.from_numpy(host if lb == 1 else host.view(np.int16)).cuda()


def _codes(env, lab, lb, k, z):
    """The packed form of lab (kdim, ncols), moved so that its last symbol is the last byte of its tensor (256 bytes of 0xFF in
    front keep the alignment)."""
    _, ops, _ = env
    kdim, ncols = lab.shape
    codes = ops.pack_sparse_codes(_dev_labels(lab, lb), kdim, ncols, k, zero_symbol=z)
    assert codes.nnz == int((lab != z).sum())
    big = torch.full((256 + codes.nbytes(),), 255, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 256 == 0
    big[256:] = codes.buf
    return ops.SparseCodes(big[256:], kdim, ncols, k, z, lb, codes.nnz)


def _call(env, x, dtype, m, codes, centers, bias, relu, half_out):
    """nnc_cbsp_h16 into sentinel-framed y and workspace (exactly the queried size); checks the frames; returns y (m, ncols) in its
    own dtype.  A half y starts an odd number of 2-byte units into its buffer, a float32 y on a 4-byte boundary that is no 8-byte one."""
    L, ops, _ = env
    kdim, ncols, lb = codes.kdim, codes.ncols, codes.label_bytes
    ws_bytes = int(L.nnc_cbsp_h16_workspace_bytes(m, kdim, ncols, lb))
    assert ws_bytes % 4 == 0
    mn = m * ncols
    units, pad = (mn, 37) if half_out else (2 * mn, 38)
    ybuf = torch.full((units + 2 * pad,), SENT16, dtype=torch.int16, device="cuda")
    wsbuf = torch.full((ws_bytes // 4 + 2 * WS_PAD,), SENT32, dtype=torch.int32, device="cuda")
    y = ybuf[pad: pad + units]
    ws_ptr = wsbuf[WS_PAD:].data_ptr() if ws_bytes else None
    dt = h16_ref.DT_CODE[dtype]
    ops.nat.check(L.nnc_cbsp_h16(x.data_ptr(), dt, m, kdim, codes.buf.data_ptr(), codes.nbytes(), lb, ncols, codes.zero_symbol, codes.nnz,
                                 centers.data_ptr(), centers.numel(), None if bias is None else bias.data_ptr(), int(relu), y.data_ptr(),
                                 dt if half_out else 0, ws_ptr, ws_bytes, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((ybuf[:pad] == SENT16).all()) and bool((ybuf[pad + units:] == SENT16).all()), "a store outside y"
    assert bool((wsbuf[:WS_PAD] == SENT32).all()) and bool((wsbuf[WS_PAD + ws_bytes // 4:] == SENT32).all()), "a store outside the workspace"
    if half_out:
        assert not bool((y == SENT16).any()), "an output left unwritten"
        return y.clone().view(_tdt(dtype)).view(m, ncols)
    assert not bool((y.view(torch.int32) == SENT32).any()), "an output left unwritten"
    return y.clone().view(torch.float32).view(m, ncols)


def _assert_exact_precondition(x, w, cz, bias):
    """Integer x, quarter-integer centres, integer bias: every partial sum of x @ W, and of the stream kernel's c_z * sum x + x @ (W -
    c_z), is a multiple of 1/4 below 2^22 / 4 in magnitude."""
    ax = np.abs(x.astype(np.float64))
    mag = ax @ (np.abs(w.astype(np.float64)) + abs(float(cz))) + abs(float(cz)) * ax.sum(axis=1, keepdims=True)
    if bias is not None:
        mag = mag + np.abs(bias.astype(np.float64))
    assert 4 * mag.max(initial=0.0) < 2.0 ** 22


def _plan(env, c, dtype):
    _, ops, cus = env
    return ops.cbsp_h16_plan(_tdt(dtype), c["m"], c["kdim"], c["ncols"], c["lb"], c["k"], cus)


# ------------------------------------------------------------------ 1. the lane maps and the vector arm of the x load
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lb", [1, 2])
def test_identity_x_returns_w_bit_for_bit(env, dtype, lb):
    """x = I (m = kdim = 64 > 16: the MFMA tile; 16-byte aligned and kdim a multiple of 8: the 16-byte x loads) and an asymmetric
    integer W decoded from a form at 30 % density with c_z != 0: y[r, c] = W[r, c] only if the decode puts every symbol at its
    (row, column) and the A, B and C / D lane maps are all right."""
    m = kdim = 64
    ncols, k, z = 96, 256, 5
    rng = np.random.RandomState(5 + lb)
    cen = rng.permutation(np.arange(-128, 128)).astype(np.float32)        # exact in bf16 and fp16; cen[z] != 0
    lab = labels_at_density(rng, kdim, ncols, k, 0.3, z)
    w = cen[lab]
    assert cen[z] != 0 and not np.array_equal(w[:, :64], w[:, :64].T)
    assert _plan(env, dict(m=m, kdim=kdim, ncols=ncols, lb=lb, k=k), dtype)["path"] == h16_ref.PATH_MFMA
    codes = _codes(env, lab, lb, k, z)
    x_t = _dev_x(np.eye(m), _tdt(dtype), False)
    assert x_t.data_ptr() % 16 == 0
    for half_out in (False, True):
        y = _call(env, x_t, dtype, m, codes, torch.from_numpy(cen).cuda(), None, False, half_out)
        assert np.array_equal(y.float().cpu().numpy(), w), (half_out, np.argwhere(y.float().cpu().numpy() != w)[:5])


# ------------------------------------------------------------------ 2. every case
def test_the_cases_hit_every_regime_at_this_device(env):
    hit = {sparse_h16_ref.regime_of(c, _plan(env, c, dtype), dtype) for c in CASES for dtype in DTYPES}
    assert hit == sparse_h16_ref.required_regimes(), sorted(sparse_h16_ref.required_regimes() - hit)


@pytest.fixture(scope="module")
def case_data(env):
    """Per case, made once and left unchanged: the labels, their packed form on the device, float data and exact data on the host."""
    out = []
    for ci, c in enumerate(CASES):
        rng = np.random.RandomState(7000 + ci)
        k, z = c["k"], 3
        lab = labels_at_density(rng, c["kdim"], c["ncols"], k, c["density"], z)
        cf = rng.standard_normal(k).astype(np.float32)
        cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
        cf[z], cen[z] = (0.0, 0.0) if c["cz_zero"] else (cf[z] + 1.5, 0.75)
        out.append(dict(lab=lab, z=z, codes=_codes(env, lab, c["lb"], k, z), cf=cf, cen=cen,
                        xf=rng.standard_normal((c["m"], c["kdim"])).astype(np.float32),
                        bf=rng.standard_normal(c["ncols"]).astype(np.float32) if c["bias"] else None,
                        x=rng.randint(-8, 9, size=(c["m"], c["kdim"])).astype(np.float32),
                        bias=rng.randint(-50, 51, size=c["ncols"]).astype(np.float32) if c["bias"] else None))
    return out


def _check_against_its_definition(env, c, dtype, codes, x_t, cen_t, bias_t, relu, tolerate_nan_bits=False):
    """One call of each output type against what defines it (see the module docstring); returns the two results."""
    _, ops, _ = env
    tdt, m = _tdt(dtype), c["m"]
    same = _same_or_both_nan if tolerate_nan_bits else _same
    got32 = _call(env, x_t, dtype, m, codes, cen_t, bias_t, relu, False)
    got16 = _call(env, x_t, dtype, m, codes, cen_t, bias_t, relu, True)
    if m > 16:
        dense = codes.to_dense()
        want32 = ops.codebook_matmul(x_t, dense, cen_t, codes.kdim, codes.ncols, bias=bias_t, relu=relu, out_dtype=torch.float32)
        want16 = ops.codebook_matmul(x_t, dense, cen_t, codes.kdim, codes.ncols, bias=bias_t, relu=relu)
    else:
        want32 = ops.sparse_codebook_matmul(x_t.float(), codes, cen_t.to(tdt).float(), bias=bias_t, relu=relu)
        want16 = want32.to(tdt)
    assert same(got32, want32) and same(got16, want16), (c, dtype)
    return got32, got16


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[sparse_h16_ref.case_id(c) for c in CASES])
def test_case(env, case_data, ci, dtype):
    _, ops, _ = env
    c, d = CASES[ci], case_data[ci]
    m, kdim, ncols, k = c["m"], c["kdim"], c["ncols"], c["k"]
    tdt, codes, lab, z, relu = _tdt(dtype), d["codes"], d["lab"], d["z"], c["relu"]
    p = _plan(env, c, dtype)
    assert p["path"] == (h16_ref.PATH_MFMA if m > 16 else h16_ref.PATH_STREAM)
    assert codes.nnz == {0.0: 0, 1.0: kdim * ncols}.get(c["density"], codes.nnz)

    # float data: x rounded to the dtype, arbitrary float32 centres (rounded by the kernel), a float32 bias
    xf_t, cf_t = _dev_x(d["xf"], tdt, c["x_view"]), torch.from_numpy(d["cf"]).cuda()
    bf_t = None if d["bf"] is None else torch.from_numpy(d["bf"]).cuda()
    got32, got16 = _check_against_its_definition(env, c, dtype, codes, xf_t, cf_t, bf_t, relu)
    assert bool(torch.isfinite(got32).all())
    # ... the same bits a second time, and through ops
    assert _same(got32, _call(env, xf_t, dtype, m, codes, cf_t, bf_t, relu, False))
    assert _same(got16, _call(env, xf_t, dtype, m, codes, cf_t, bf_t, relu, True))
    assert _same(got32, ops.sparse_codebook_matmul(xf_t, codes, cf_t, bias=bf_t, relu=relu, out_dtype=torch.float32))
    assert _same(got16, ops.sparse_codebook_matmul(xf_t, codes, cf_t, bias=bf_t, relu=relu))

    # an Inf and a NaN in x, each against a row of W that holds a skipped and (density > 0) a stored position
    xn = round_to(d["xf"], dtype)
    xn[0, 0], xn[m - 1, kdim - 1], xn[min(1, m - 1), kdim // 2] = np.inf, np.nan, -np.inf
    n32, _ = _check_against_its_definition(env, c, dtype, codes, _dev_x(xn, tdt, c["x_view"]), cf_t, bf_t, relu, tolerate_nan_bits=True)
    if m > 16:   # W_h holds an entry at every position: the NaN of row m - 1 reaches every column, and ReLU keeps it
        assert bool(torch.isnan(n32[m - 1]).all())
    # c_z == 0, up to 16 rows: a skipped weight is absent, so an Inf that meets only skipped positions in a column leaves it finite
    if m <= 16 and c["cz_zero"] and np.any(lab[0] == z):
        xi = round_to(d["xf"], dtype)
        xi[0, 0] = np.inf
        i32, _ = _check_against_its_definition(env, c, dtype, codes, _dev_x(xi, tdt, c["x_view"]), cf_t, bf_t, relu)
        skipped = torch.from_numpy(lab[0] == z).cuda()
        assert bool(torch.isfinite(i32[0][skipped]).all()) and (relu or not bool(torch.isfinite(i32[0][~skipped]).any()))

    # exact data: the float64 product with the decoded W bit for bit, in float32 and (rounded once) in half
    x, cen, bias = d["x"], d["cen"], d["bias"]
    w = cen[lab]
    _assert_exact_precondition(x, w, cen[z], bias)
    want = matmul64(x, w, bias)
    ref = (relu_like_torch(want) if relu else want).astype(np.float32)
    x_t, cen_t = _dev_x(x, tdt, c["x_view"]), torch.from_numpy(cen).cuda()
    bias_t = None if bias is None else torch.from_numpy(bias).cuda()
    e32, e16 = _check_against_its_definition(env, c, dtype, codes, x_t, cen_t, bias_t, relu)
    assert np.array_equal(e32.cpu().numpy(), ref), (c, dtype)
    assert np.array_equal(e16.float().cpu().numpy(), round_to(ref, dtype)), (c, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kdim,ncols,lb,k,cz", [(33, 50, 1, 256, 0.0), (64, 129, 2, 1040, 0.5), (300, 129, 2, 300, -0.25), (1001, 200, 1, 17, 0.0)])
def test_m16_and_m17_rows_agree(env, dtype, kdim, ncols, lb, k, cz):
    """The first 16 rows through the stream kernel (m = 16) and through the MFMA tile (m = 17), on the same exact data: the same
    bits, float32 and half, whichever formula formed them."""
    rng = np.random.RandomState(kdim)
    z = 1
    lab = labels_at_density(rng, kdim, ncols, k, 0.3, z)
    x = rng.randint(-8, 9, size=(17, kdim)).astype(np.float32)
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    cen[z] = cz
    bias = rng.randint(-50, 51, size=ncols).astype(np.float32)
    _assert_exact_precondition(x, cen[lab], cz, bias)
    codes = _codes(env, lab, lb, k, z)
    x_t, cen_t, bias_t = _dev_x(x, _tdt(dtype), False), torch.from_numpy(cen).cuda(), torch.from_numpy(bias).cuda()
    for half_out in (False, True):
        y16 = _call(env, x_t[:16], dtype, 16, codes, cen_t, bias_t, True, half_out)
        y17 = _call(env, x_t, dtype, 17, codes, cen_t, bias_t, True, half_out)
        assert _same(y16, y17[:16]), half_out


# ------------------------------------------------------------------ 3. values
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,lb,k,z", [(5, 1, 17, 3), (5, 2, 257, 300), (40, 1, 17, 200), (40, 2, 257, 3)])
def test_an_index_past_k_reads_zero(env, dtype, m, lb, k, z):
    """stored symbols >= K, and a skipped symbol >= K (z = 200 of K = 17, z = 300 of K = 257): all of them weigh 0"""
    kdim, ncols = 70, 77
    rng = np.random.RandomState(m + z)
    top = 255 if lb == 1 else 65535
    lab = labels_at_density(rng, kdim, ncols, k, 0.4, min(z, k - 1))
    if z >= k:
        lab[lab == k - 1] = z
    lab[2, ::3], lab[9, 1::2], lab[40, :] = top, k, k + 3
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    if z < k:
        cen[z] = 1.25
    x = rng.randint(-8, 9, size=(m, kdim)).astype(np.float32)
    w = np.append(cen, np.float32(0.0))[np.minimum(lab, k)]
    _assert_exact_precondition(x, w, cen[z] if z < k else 0.0, None)
    want = matmul64(x, w).astype(np.float32)
    codes = _codes(env, lab, lb, k, z)
    x_t, cen_t = _dev_x(x, _tdt(dtype), True), torch.from_numpy(cen).cuda()
    assert np.array_equal(_call(env, x_t, dtype, m, codes, cen_t, None, False, False).cpu().numpy(), want)
    assert np.array_equal(_call(env, x_t, dtype, m, codes, cen_t, None, False, True).float().cpu().numpy(), round_to(want, dtype))


@pytest.mark.parametrize("m", [4, 40])
def test_fp16_centre_beyond_the_range_acts_as_inf(env, m):
    """A centre of 1e5 is Inf in fp16, as centers.to(torch.float16) makes it (and 1e5 rounded in bf16); -7e4 is -Inf."""
    kdim, ncols, k, z = 40, 50, 6, 5
    rng = np.random.RandomState(m)
    cen = np.array([1e5, -7e4, 0.5, -2.0, 65520.0 - 16.1, 0.0], dtype=np.float32)
    lab = rng.randint(2, 4, size=(kdim, ncols))
    lab[rng.random_sample((kdim, ncols)) < 0.5] = z
    lab[3, 0::4], lab[5, 1::4], lab[7, 2::4] = 0, 1, 4
    x = rng.randint(1, 3, size=(m, kdim)).astype(np.float32)
    x[1, 3] = 0.0                                                     # 0 * Inf = NaN in row 1
    codes, cen_t = _codes(env, lab, 1, k, z), torch.from_numpy(cen).cuda()
    for dtype in DTYPES:
        wh = torch.from_numpy(cen).to(_tdt(dtype)).float().numpy()[lab]
        assert np.isinf(wh).any() == (dtype == "fp16")
        want = matmul64(x, wh).astype(np.float32)
        y = _call(env, _dev_x(x, _tdt(dtype), False), dtype, m, codes, cen_t, None, False, False).cpu().numpy()
        if dtype == "fp16":
            assert np.isposinf(want).any() and np.isneginf(want).any() and np.isnan(want).any()
            assert np.array_equal(y, want, equal_nan=True)
        else:
            assert np.isfinite(want).all() and np.allclose(y, want, rtol=1e-5, atol=0)


def test_degenerate_shapes_and_python_errors(env):
    """m = 0 and ncols = 0 write nothing; kdim = 0 writes the bias (ReLU applied), in float32 and in half; the dtype rules of ops"""
    _, ops, _ = env
    cen_t = torch.ones(4, device="cuda")
    bias = np.array([-1.5, 2.25, 0.0, 1000.0, -3.0], dtype=np.float32)
    bias_t = torch.from_numpy(bias).cuda()
    empty = ops.pack_sparse_codes(torch.zeros(0, dtype=torch.uint8, device="cuda"), 0, 5, 4, zero_symbol=0)
    codes = ops.pack_sparse_codes(torch.zeros(7 * 5, dtype=torch.uint8, device="cuda"), 7, 5, 4, zero_symbol=0)
    for dtype in DTYPES:
        for m in (3, 20):
            x_t = torch.zeros((m, 0), dtype=_tdt(dtype), device="cuda")
            for half_out in (False, True):
                y = _call(env, x_t, dtype, m, empty, cen_t, bias_t, True, half_out)
                assert np.array_equal(y.float().cpu().numpy(), np.tile(np.maximum(bias, 0), (m, 1)))
        assert ops.sparse_codebook_matmul(torch.zeros((0, 7), dtype=_tdt(dtype), device="cuda"), codes, cen_t).shape == (0, 5)
        x_t = torch.zeros((2, 7), dtype=_tdt(dtype), device="cuda")
        assert ops.sparse_codebook_matmul(x_t, codes, cen_t).dtype == _tdt(dtype)
        assert ops.sparse_codebook_matmul(x_t, codes, cen_t, out_dtype=torch.float32).dtype == torch.float32
        other = torch.float16 if dtype == "bf16" else torch.bfloat16
        for kw in (dict(out_dtype=other), dict(out_dtype=torch.float64), dict(bias=bias_t.to(_tdt(dtype))), dict(centers=cen_t.to(_tdt(dtype)))):
            args = dict(centers=cen_t, bias=bias_t, out_dtype=None)
            args.update(kw)
            with pytest.raises(TypeError):
                ops.sparse_codebook_matmul(x_t, codes, args["centers"], bias=args["bias"], out_dtype=args["out_dtype"])
        with pytest.raises(RuntimeError, match="inference only"):
            ops.sparse_codebook_matmul(x_t.clone().requires_grad_(), codes, cen_t)
    with pytest.raises(TypeError):
        ops.sparse_codebook_matmul(torch.zeros((2, 7), dtype=torch.float64, device="cuda"), codes, cen_t)
    with pytest.raises(TypeError):
        ops.sparse_codebook_matmul(torch.zeros((2, 7), device="cuda"), codes, cen_t, out_dtype=torch.bfloat16)
    assert ops.sparse_codebook_matmul(torch.zeros((2, 7), device="cuda"), codes, cen_t, out_dtype=torch.float32).dtype == torch.float32


# ------------------------------------------------------------------ 4. layers
def _layer_data(rng, kdim, ncols, k):
    lab = labels_at_density(rng, kdim, ncols, k, 0.3, 0).ravel().astype(np.uint8)
    cen = rng.standard_normal(k).astype(np.float32)
    cen[0] = 0.0
    bias = rng.standard_normal(ncols).astype(np.float32)
    return torch.from_numpy(lab).cuda(), torch.from_numpy(cen).cuda(), torch.from_numpy(bias).cuda()


@pytest.mark.parametrize("dtype", DTYPES)
def test_dense_layers_with_half_inputs_equal_the_op_and_chain_in_half(env, dtype):
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    tdt = _tdt(dtype)
    rng = np.random.RandomState(11)
    l1 = compressed.SparseCompressedDense.from_codes(64, 48, *_layer_data(rng, 64, 48, 9), torch.relu, half_inputs=True)
    l2 = compressed.SparseCompressedDense.from_codes(48, 10, *_layer_data(rng, 48, 10, 9), None, None, True)
    assert l1.half_inputs and l2.half_inputs
    for m in (3, 40):
        x = torch.from_numpy(rng.standard_normal((m, 64)).astype(np.float32)).cuda().to(tdt)
        with torch.no_grad():
            h = l1(x)
            y = l2(h)
        assert h.dtype == tdt and y.dtype == tdt
        assert _same(h, ops.sparse_codebook_matmul(x, l1.codes, l1.centers, bias=l1.bias, relu=True))
        assert _same(y, ops.sparse_codebook_matmul(h, l2.codes, l2.centers, bias=l2.bias))
        with pytest.raises(RuntimeError, match="inference only"):
            l1(x.clone().requires_grad_())


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv2d_with_half_inputs_equals_the_op_and_chunks_by_the_element_size(env, dtype, monkeypatch):
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    tdt = _tdt(dtype)
    rng = np.random.RandomState(12)
    lab_t, cen_t, bias_t = _layer_data(rng, 3 * 3 * 2, 4, 9)
    layer = compressed.SparseCompressedConv2D.from_codes(3, 2, 4, 1, lab_t, cen_t, bias_t, torch.relu, half_inputs=True)
    x = torch.from_numpy(rng.standard_normal((7, 6, 5, 2)).astype(np.float32)).cuda().to(tdt)
    with torch.no_grad():
        whole = layer(x)
    assert whole.dtype == tdt and whole.shape == (7, 6, 5, 4)
    patches = compressed.conv_patches(x, 3, 1).contiguous()
    assert _same(whole.reshape(-1, 4), ops.sparse_codebook_matmul(patches, layer.codes, layer.centers, bias=layer.bias, relu=True).reshape(-1, 4))
    per_image = 6 * 5 * 3 * 3 * 2 * 2           # 2 bytes an element
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
        empty = layer(torch.empty(0, 6, 5, 2, dtype=tdt, device="cuda"))
    assert empty.shape == (0, 6, 5, 4) and empty.dtype == tdt


def _small_dense_network(rng):
    """LeNet-300-100 with a five-centre codebook per tensor, about 14 % of the kernels stored: no fit needed"""
    from types import SimpleNamespace

    from neural_network_compression_amd.neural_networks.le_net_300_100 import LeNet300100

    net = LeNet300100().cuda()
    cen = np.array([0.0, 0.5, -0.5, 1.0, -1.0], dtype=np.float32)
    models = {}
    for layer in net.get_config().values():
        kl = rng.choice(5, size=layer.kernel.numel(), p=[0.86, 0.035, 0.035, 0.035, 0.035])
        bl = rng.choice(5, size=layer.bias.numel(), p=[0.4, 0.15, 0.15, 0.15, 0.15])
        kt, bt = torch.from_numpy(kl.astype(np.uint8)).cuda(), torch.from_numpy(bl.astype(np.uint8)).cuda()
        layer.set_weights([torch.from_numpy(cen[kl]).cuda().view(layer.kernel.shape), torch.from_numpy(cen[bl]).cuda()])
        models[layer] = [SimpleNamespace(cluster_centers_=cen.reshape(-1, 1), labels_compact_=kt),
                         SimpleNamespace(cluster_centers_=cen.reshape(-1, 1), labels_compact_=bt)]
    return net, models


def test_compress_network_with_sparse_half_inputs(env):
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    net, models = _small_dense_network(np.random.RandomState(31))
    plain = compressed.compress_network(net, models, sparse=True)
    half = compressed.compress_network(net, models, sparse=True, sparse_half_inputs=True)
    x = (torch.rand(40, 784, device="cuda") < 0.05).float()
    for tdt in (torch.bfloat16, torch.float16):
        xh = x.to(tdt)
        with torch.no_grad():
            y = half(xh)
            h = xh
            for name, layer in half.get_config().items():
                assert isinstance(layer, compressed.SparseCompressedDense) and layer.half_inputs and not plain.get_config()[name].half_inputs
                h = ops.sparse_codebook_matmul(h, layer.codes, layer.centers, bias=layer.bias, relu=layer._fused_relu)
        assert y.dtype == tdt and _same(y, h)
        with torch.no_grad(), pytest.raises(TypeError, match="byte form"):
            plain(xh)
    with torch.no_grad():
        assert _same(half(x), plain(x))                               # a float32 input takes the float32 path, option or not
    # "auto" picks what it picked, by resident bytes; the layers it leaves in the byte form take half inputs anyway
    auto, auto_half = compressed.compress_network(net, models, sparse="auto"), compressed.compress_network(net, models, sparse="auto", sparse_half_inputs=True)
    assert [type(l) for l in auto.get_config().values()] == [type(l) for l in auto_half.get_config().values()]
    assert compressed.compressed_nbytes(auto) == compressed.compressed_nbytes(auto_half)
    with torch.no_grad():
        assert auto_half(x.to(torch.bfloat16)).dtype == torch.bfloat16


# ------------------------------------------------------------------ 5. unchanged behaviour
def test_without_the_option_half_inputs_raise_and_float32_keeps_its_bits(env):
    """The layers built the plain way raise TypeError on a half input; a float32 x through every sparse layer, built either way, is
    nnc_cbsp_f32 called directly, bit for bit, at m on both sides of 16."""
    from neural_network_compression_amd import compressed

    L, ops, _ = env
    rng = np.random.RandomState(13)
    kdim, ncols, k = 64, 48, 9
    data = _layer_data(rng, kdim, ncols, k)
    conv_data = _layer_data(rng, 3 * 3 * 2, 4, k)
    for tdt in (torch.bfloat16, torch.float16):
        with torch.no_grad(), pytest.raises(TypeError, match="byte form"):
            compressed.SparseCompressedDense.from_codes(kdim, ncols, *data, None)(torch.zeros(3, kdim, dtype=tdt, device="cuda"))
        with torch.no_grad(), pytest.raises(TypeError, match="byte form"):
            compressed.SparseCompressedConv2D.from_codes(3, 2, 4, 1, *conv_data, None)(torch.zeros(2, 6, 6, 2, dtype=tdt, device="cuda"))

    def direct(x2, layer, relu):
        m = x2.shape[0]
        codes = layer.codes
        ws_bytes = int(L.nnc_cbsp_workspace_bytes(m, codes.kdim, codes.ncols, codes.label_bytes))
        ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device="cuda")
        y = torch.empty((m, codes.ncols), dtype=torch.float32, device="cuda")
        ops.nat.check(L.nnc_cbsp_f32(x2.data_ptr(), m, codes.kdim, codes.buf.data_ptr(), codes.nbytes(), codes.label_bytes, codes.ncols,
                                     codes.zero_symbol, codes.nnz, layer.centers.data_ptr(), layer.centers.numel(), layer.bias.data_ptr(), int(relu),
                                     y.data_ptr(), ws.data_ptr() if ws_bytes else None, ws_bytes, torch.cuda.current_stream().cuda_stream))
        return y

    for half_inputs in (False, True):
        dense = compressed.SparseCompressedDense.from_codes(kdim, ncols, *data, torch.relu, half_inputs=half_inputs)
        conv = compressed.SparseCompressedConv2D.from_codes(3, 2, 4, 1, *conv_data, None, half_inputs=half_inputs)
        for m in (5, 40):
            x = torch.from_numpy(rng.standard_normal((m, kdim)).astype(np.float32)).cuda()
            with torch.no_grad():
                assert _same(dense(x), direct(x, dense, True))
            assert _same(ops.sparse_codebook_matmul(x, dense.codes, dense.centers, bias=dense.bias, relu=True), direct(x, dense, True))
        for n in (1, 3):                                              # 6 * 5 = 30 patches an image: m = 30 and 90... and 1 x 2 x 2 = 4
            xc = torch.from_numpy(rng.standard_normal((n, 6, 5, 2)).astype(np.float32)).cuda()
            with torch.no_grad():
                got = conv(xc)
            assert _same(got.reshape(-1, 4), direct(compressed.conv_patches(xc, 3, 1).contiguous().reshape(-1, 18), conv, False))
        xc = torch.from_numpy(rng.standard_normal((1, 2, 2, 2)).astype(np.float32)).cuda()
        with torch.no_grad():
            assert _same(conv(xc).reshape(-1, 4), direct(compressed.conv_patches(xc, 3, 1).contiguous().reshape(-1, 18), conv, False))
