"""The codebook matmul on bf16 / fp16 activations (nnc_cbmm_h16, csrc/nnc_cbmm_h16.hip) against float64
NumPy, through the raw C ABI with buffers the test owns, and through ops.codebook_matmul and the layers (run with -m gpu).

The lane maps of the MFMA tile first (x = identity, an asymmetric W); then every case of tests/helpers/h16_ref.py with both
dtypes: exact data bit for bit (float32 output, with and without ReLU; half output = that result rounded once), float data within
the float32 bound, every call into sentinel-framed y and workspace slices (2-byte granularity for a half y) and repeated for the
same bits; then non-finite inputs and the fp16 range, NaN-filled memory directly behind x and the labels, and the layers.

The float bound: the products of two bf16 or two fp16 values are exact in float32; a result is the sum of at most kdim products, the
split partials and the bias, so at most kdim + splits + 1 additions each err by at most one float32 ulp (2^-23 relative; a whole ulp
allows for truncation inside the MFMA) of a partial sum <= mag = |x| @ |W_h| + |bias|: err <= (kdim + splits + 2) 2^-23 mag.  A half
output adds half an ulp of the dtype at |ref| (h16_ref.half_ulp: 2^-9 (bf16) / 2^-12 (fp16) of the upper end of ref's binade,
2^-25 below fp16's normal range)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import cbmm_ref, h16_ref  # noqa: E402
from tests.helpers.cbmm_ref import matmul64, relu_like_torch  # noqa: E402
from tests.helpers.h16_ref import CASES, DTYPES, round_to  # noqa: E402

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


def _dev(host, tdtype, view):
    """host float32 values -> device tensor of ``tdtype`` (the values must be exact in it, or are rounded by torch);
    ``view``: as buf[1:] of a one-longer buffer (aligned to the element size and no further)."""
    t = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).to(tdtype)
    if not view:
        return t.cuda()
    buf = torch.zeros(t.numel() + 1, dtype=tdtype, device="cuda")
    buf[1:] = t.reshape(-1).cuda()
    return buf[1:].view(t.shape)


def _dev_labels(lab, lb, off, tail=None):
    """The indices as uint8 / int16 starting ``off`` elements into a buffer that has 16 spare bytes after them (``tail``: their
    fill)."""
    dt = torch.uint8 if lb == 1 else torch.int16
    host = lab.astype(np.uint8) if lb == 1 else lab.astype(np.uint16).view(np.int16)
    buf = torch.zeros(off + host.size + 16 // lb, dtype=dt, device="cuda")
    if tail is not None:
        buf.fill_(tail)
    buf[off: off + host.size] = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    return buf[off: off + host.size]


def _call(env, x, dtype, m, kdim, labels, lb, ncols, centers, k, bias, relu, half_out):
    """nnc_cbmm_h16 into sentinel-framed y and workspace (exactly the queried size); checks the frames; returns y as float32
    (device, m x ncols) and its raw bits.  A half y starts an odd number of 2-byte units into its buffer, a float32 y on a 4-byte
    boundary that is no 8-byte one."""
    L, ops, _ = env
    ws_bytes = int(L.nnc_cbmm_h16_workspace_bytes(m, kdim, ncols, lb))
    assert ws_bytes % 4 == 0
    mn = m * ncols
    units, pad = (mn, 37) if half_out else (2 * mn, 38)
    ybuf = torch.full((units + 2 * pad,), SENT16, dtype=torch.int16, device="cuda")
    wsbuf = torch.full((ws_bytes // 4 + 2 * WS_PAD,), SENT32, dtype=torch.int32, device="cuda")
    y = ybuf[pad: pad + units]
    ws_ptr = wsbuf[WS_PAD:].data_ptr() if ws_bytes else None
    dt = h16_ref.DT_CODE[dtype]
    ops.nat.check(L.nnc_cbmm_h16(x.data_ptr(), dt, m, kdim, labels.data_ptr(), lb, ncols, centers.data_ptr(), k,
                                 None if bias is None else bias.data_ptr(), int(relu), y.data_ptr(), dt if half_out else 0, ws_ptr, ws_bytes,
                                 torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((ybuf[:pad] == SENT16).all()) and bool((ybuf[pad + units:] == SENT16).all()), "a store outside y"
    assert bool((wsbuf[:WS_PAD] == SENT32).all()) and bool((wsbuf[WS_PAD + ws_bytes // 4:] == SENT32).all()), "a store outside the workspace"
    if half_out:
        assert not bool((y == SENT16).any()), "an output left unwritten"
        return y.view(_tdt(dtype)).view(m, ncols).float(), y.clone()
    assert not bool((y.view(torch.int32) == SENT32).any()), "an output left unwritten"
    return y.view(torch.float32).view(m, ncols).clone(), y.clone()


def _assert_exact_precondition(x, w, bias):
    """Integer x, quarter-integer centres, integer bias: every partial sum is a multiple of 1/4 below 2^22 / 4 in magnitude."""
    mag = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64))
    if bias is not None:
        mag = mag + np.abs(bias.astype(np.float64))
    assert 4 * mag.max(initial=0.0) < 2.0 ** 22


def _plan(env, c, dtype, addr):
    _, ops, cus = env
    return ops.cbmm_h16_plan(_tdt(dtype), c["m"], c["kdim"], c["ncols"], c["lb"], c["k"], cus, addr)


# ------------------------------------------------------------------ 1. the lane maps
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lb", [1, 2])
def test_identity_x_returns_w_bit_for_bit(env, dtype, lb):
    """x = I (m = kdim = 64 > 16: the MFMA tile) and an asymmetric integer W (K = 256 distinct centres, random indices, ncols != m):
    y[r, c] = W[r, c] only if the A, B and C / D lane maps are all right."""
    _, ops, cus = env
    m = kdim = 64
    ncols, k = 96, 256
    rng = np.random.RandomState(5)
    cen = rng.permutation(np.arange(-128, 128)).astype(np.float32)        # exact in bf16 and fp16
    lab = rng.randint(0, k, size=(kdim, ncols))
    w = cen[lab]
    assert not np.array_equal(w[:, :64], w[:, :64].T)
    assert ops.cbmm_h16_plan(_tdt(dtype), m, kdim, ncols, lb, k, cus)["path"] == h16_ref.PATH_MFMA
    x_t, cen_t, lab_t = _dev(np.eye(m), _tdt(dtype), False), torch.from_numpy(cen).cuda(), _dev_labels(lab.ravel(), lb, 0)
    for half_out in (False, True):
        y, _ = _call(env, x_t, dtype, m, kdim, lab_t, lb, ncols, cen_t, k, None, False, half_out)
        assert np.array_equal(y.cpu().numpy(), w), (half_out, np.argwhere(y.cpu().numpy() != w)[:5])


# ------------------------------------------------------------------ 2, 3, 5. every case: exact data, float data, frames
def test_the_cases_hit_every_regime_at_this_device(env):
    hit = set()
    for c in CASES:
        for dtype in DTYPES:
            p = _plan(env, c, dtype, 4096 + c["off"] * c["lb"])
            hit.add(h16_ref.regime_of(c, p, dtype))
            assert p["splits"] > 1 or c["kdim"] not in h16_ref.MUST_SPLIT_KDIMS, (c, p)
    assert hit == h16_ref.required_regimes(), sorted(h16_ref.required_regimes() - hit)


@pytest.fixture(scope="module")
def case_data():
    """Per case, made once: labels, exact data and float data on the host (the float64 references are formed per dtype)."""
    out = []
    for ci, c in enumerate(CASES):
        rng = np.random.RandomState(9000 + ci)
        k = c["k"]
        out.append(dict(lab=rng.randint(0, k, size=c["kdim"] * c["ncols"]),
                        x=rng.randint(-8, 9, size=(c["m"], c["kdim"])).astype(np.float32),
                        cen=(rng.randint(-16, 17, size=k) / 4.0).astype(np.float32),
                        bias=rng.randint(-50, 51, size=c["ncols"]).astype(np.float32) if c["bias"] else None,
                        xf=rng.standard_normal((c["m"], c["kdim"])).astype(np.float32),
                        cf=rng.standard_normal(k).astype(np.float32),
                        bf=rng.standard_normal(c["ncols"]).astype(np.float32) if c["bias"] else None))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[h16_ref.case_id(c) for c in CASES])
def test_case(env, case_data, ci, dtype):
    c, d = CASES[ci], case_data[ci]
    m, kdim, ncols, lb, k = c["m"], c["kdim"], c["ncols"], c["lb"], c["k"]
    tdt = _tdt(dtype)
    lab_t = _dev_labels(d["lab"], lb, c["off"])
    p = _plan(env, c, dtype, lab_t.data_ptr())
    assert h16_ref.regime_of(c, p, dtype) == h16_ref.regime_of(c, _plan(env, c, dtype, 4096 + c["off"] * lb), dtype)

    # exact data: the float64 result bit for bit; the half output is that result rounded once; the same bits a second time
    x, cen, bias = d["x"], d["cen"], d["bias"]
    w = cen[d["lab"]].reshape(kdim, ncols)
    _assert_exact_precondition(x, w, bias)
    want = x.astype(np.float64) @ w.astype(np.float64) + (0 if bias is None else bias.astype(np.float64))
    x_t, cen_t = _dev(x, tdt, c["x_view"]), _dev(cen, torch.float32, False)
    bias_t = None if bias is None else _dev(bias, torch.float32, c["bias_view"])
    for relu in (False, True):
        ref = (relu_like_torch(want) if relu else want).astype(np.float32)
        y, bits = _call(env, x_t, dtype, m, kdim, lab_t, lb, ncols, cen_t, k, bias_t, relu, False)
        assert np.array_equal(y.cpu().numpy(), ref), (c, relu)
        yh, bits_h = _call(env, x_t, dtype, m, kdim, lab_t, lb, ncols, cen_t, k, bias_t, relu, True)
        assert np.array_equal(yh.cpu().numpy(), round_to(ref, dtype)), (c, relu)
    assert torch.equal(bits, _call(env, x_t, dtype, m, kdim, lab_t, lb, ncols, cen_t, k, bias_t, True, False)[1])
    assert torch.equal(bits_h, _call(env, x_t, dtype, m, kdim, lab_t, lb, ncols, cen_t, k, bias_t, True, True)[1])

    # float data: x rounded to the dtype, arbitrary float32 centres (rounded by the kernel as centers.to(dtype)), float32 bias
    xf = round_to(d["xf"], dtype)
    wh = torch.from_numpy(d["cf"]).to(tdt).float().numpy()[d["lab"]].reshape(kdim, ncols)
    bf = d["bf"]
    ref = matmul64(xf, wh, bf)
    mag = np.abs(xf.astype(np.float64)) @ np.abs(wh.astype(np.float64)) + (0 if bf is None else np.abs(bf.astype(np.float64)))
    bound = (kdim + p["splits"] + 2) * 2.0 ** -23 * mag
    xf_t, cf_t = _dev(xf, tdt, c["x_view"]), _dev(d["cf"], torch.float32, False)
    bf_t = None if bf is None else _dev(bf, torch.float32, c["bias_view"])
    y, bits = _call(env, xf_t, dtype, m, kdim, lab_t, lb, ncols, cf_t, k, bf_t, False, False)
    err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"h16 float32 output: {h16_ref.case_id(c)} {dtype}: largest err / bound = {worst:.4f}")
    assert np.all(err <= bound), (c, dtype, worst)
    yh, bits_h = _call(env, xf_t, dtype, m, kdim, lab_t, lb, ncols, cf_t, k, bf_t, False, True)
    err_h = np.abs(yh.cpu().numpy().astype(np.float64) - ref)
    bound_h = bound + h16_ref.half_ulp(ref, dtype)
    assert np.all(err_h <= bound_h), (c, dtype, float((err_h / bound_h).max()))
    assert torch.equal(bits, _call(env, xf_t, dtype, m, kdim, lab_t, lb, ncols, cf_t, k, bf_t, False, False)[1])
    assert torch.equal(bits_h, _call(env, xf_t, dtype, m, kdim, lab_t, lb, ncols, cf_t, k, bf_t, False, True)[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kdim,ncols,lb,k", [(33, 50, 1, 256), (300, 129, 2, 300), (1001, 200, 1, 17)])
def test_m16_and_m17_rows_agree(env, dtype, kdim, ncols, lb, k):
    """The first 16 rows through the stream kernel (m = 16) and through the MFMA tile (m = 17), on the same exact data: the same
    bits, float32 and half."""
    rng = np.random.RandomState(kdim)
    lab = rng.randint(0, k, size=kdim * ncols)
    x = rng.randint(-8, 9, size=(17, kdim)).astype(np.float32)
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    bias = rng.randint(-50, 51, size=ncols).astype(np.float32)
    _assert_exact_precondition(x, cen[lab].reshape(kdim, ncols), bias)
    x_t, cen_t, bias_t, lab_t = _dev(x, _tdt(dtype), False), _dev(cen, torch.float32, False), _dev(bias, torch.float32, False), _dev_labels(lab, lb, 1)
    for half_out in (False, True):
        y16, _ = _call(env, x_t[:16], dtype, 16, kdim, lab_t, lb, ncols, cen_t, k, bias_t, True, half_out)
        y17, _ = _call(env, x_t, dtype, 17, kdim, lab_t, lb, ncols, cen_t, k, bias_t, True, half_out)
        assert torch.equal(y16.view(torch.int32), y17[:16].view(torch.int32)), half_out


# ------------------------------------------------------------------ 4. non-finite inputs and the fp16 range
# (m, kdim, ncols, lb, k, path, split): the stream and MFMA kernels, each direct and through the split-K combine
NONFINITE = [(3, 20, 77, 1, 17, 1, False), (5, 700, 50, 2, 300, 1, True), (16, 600, 33, 1, 256, 1, True),
             (40, 100, 129, 1, 17, 5, False), (17, 300, 50, 2, 1040, 5, True)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,kdim,ncols,lb,k,path,split", NONFINITE)
def test_nonfinite_inputs_propagate_and_relu_keeps_nan(env, dtype, m, kdim, ncols, lb, k, path, split):
    """NaN and +-Inf in x, NaN in the bias; Inf against the centre that is exactly 0 gives NaN; an index >= K reads 0 (and Inf
    against it NaN).  The result equals the float64 one (NaN where it is NaN); the fused ReLU maps -Inf to 0 and keeps NaN."""
    _, ops, cus = env
    rng = np.random.RandomState(m * 1000 + kdim)
    lab = rng.randint(0, k, size=(kdim, ncols))
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    cen[0] = 0.0
    lab[2, ::3] = 0                         # row 2 meets +Inf (below) against the exact 0 centre in every third column
    top = 255 if lb == 1 else 65535
    if k <= top:
        lab[2, 1::3] = top                  # ... and against an index >= K in the next ones
        lab[9, :] = min(top, k + 3)
    x = rng.randint(-8, 9, size=(m, kdim)).astype(np.float32)
    x[0, 1] = np.nan
    x[1, 2] = np.inf
    x[m - 1, 5] = -np.inf
    x[m - 1, kdim - 1] = np.inf
    if m > 2:
        x[2, 7] = -np.inf
    bias = rng.randint(-50, 51, size=ncols).astype(np.float32)
    bias[4] = np.nan
    w = np.append(cen, np.float32(0.0))[np.minimum(lab, k)]
    _assert_exact_precondition(np.where(np.isfinite(x), x, 0), w, np.where(np.isfinite(bias), bias, 0))
    lab_t = _dev_labels(lab.ravel(), lb, 0)
    p = ops.cbmm_h16_plan(_tdt(dtype), m, kdim, ncols, lb, k, cus, lab_t.data_ptr())
    assert p["path"] == path and (p["splits"] > 1) == split, p
    want = matmul64(x, w, bias)
    assert np.isnan(want).any() and np.isposinf(want).any() and np.isneginf(want).any()
    x_t, cen_t, bias_t = _dev(x, _tdt(dtype), False), _dev(cen, torch.float32, False), _dev(bias, torch.float32, False)
    for relu in (False, True):
        ref = (relu_like_torch(want) if relu else want).astype(np.float32)
        for half_out in (False, True):
            y = _call(env, x_t, dtype, m, kdim, lab_t, lb, ncols, cen_t, k, bias_t, relu, half_out)[0].cpu().numpy()
            r = round_to(ref, dtype) if half_out else ref
            assert np.array_equal(y, r, equal_nan=True), (relu, half_out, np.argwhere(~((y == r) | (np.isnan(y) & np.isnan(r))))[:5])


@pytest.mark.parametrize("m", [4, 40])
def test_fp16_centre_beyond_the_range_acts_as_inf(env, m):
    """A centre of 1e5 is Inf in fp16, as centers.to(torch.float16) makes it (and 1e5 rounded in bf16); -7e4 is -Inf."""
    kdim, ncols, k = 40, 50, 5
    rng = np.random.RandomState(m)
    cen = np.array([1e5, -7e4, 0.5, -2.0, 65520.0 - 16.1], dtype=np.float32)
    lab = rng.randint(2, 4, size=(kdim, ncols))
    lab[3, 0::4], lab[5, 1::4], lab[7, 2::4] = 0, 1, 4
    x = rng.randint(1, 3, size=(m, kdim)).astype(np.float32)
    x[1, 3] = 0.0                                                     # 0 * Inf = NaN in row 1
    lab_t, cen_t = _dev_labels(lab.ravel(), 1, 0), torch.from_numpy(cen).cuda()
    for dtype in DTYPES:
        wh = torch.from_numpy(cen).to(_tdt(dtype)).float().numpy()[lab]
        assert np.isinf(wh).any() == (dtype == "fp16")
        want = matmul64(x, wh).astype(np.float32)
        y = _call(env, _dev(x, _tdt(dtype), False), dtype, m, kdim, lab_t, 1, ncols, cen_t, k, None, False, False)[0].cpu().numpy()
        if dtype == "fp16":
            assert np.isposinf(want).any() and np.isneginf(want).any() and np.isnan(want).any()
            assert np.array_equal(y, want, equal_nan=True)
        else:
            assert np.isfinite(want).all() and np.allclose(y, want, rtol=1e-5, atol=0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,kdim,ncols,lb", [(3, 37, 50, 1), (16, 301, 129, 2), (17, 1, 1, 1), (33, 37, 50, 2), (130, 301, 129, 1), (40, 1001, 16, 1)])
def test_nan_filled_memory_behind_x_and_the_labels_changes_nothing(env, dtype, m, kdim, ncols, lb):
    """x and the labels end directly in front of NaN bit patterns (0xFFFF units: a NaN in both dtypes, an index >= K): a k tail or
    a column tail padded from memory would turn the outputs into NaN or change them."""
    k = 200 if lb == 1 else 300
    rng = np.random.RandomState(kdim + m)
    lab = rng.randint(0, k, size=kdim * ncols)
    x = rng.randint(-8, 9, size=(m, kdim)).astype(np.float32)
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    w = cen[lab].reshape(kdim, ncols)
    _assert_exact_precondition(x, w, None)
    want = (x.astype(np.float64) @ w.astype(np.float64)).astype(np.float32)
    xbuf = torch.full((1 + m * kdim + 64,), -1, dtype=torch.int16, device="cuda")
    x_t = xbuf[1: 1 + m * kdim].view(_tdt(dtype))
    x_t.copy_(torch.from_numpy(x).to(_tdt(dtype)).reshape(-1))
    assert bool(torch.isnan(xbuf.view(_tdt(dtype))[1 + m * kdim:].float()).all())
    lab_t = _dev_labels(lab, lb, 1, tail=-1 if lb == 2 else 255)
    y = _call(env, x_t.view(m, kdim), dtype, m, kdim, lab_t, lb, ncols, torch.from_numpy(cen).cuda(), k, None, False, False)[0]
    assert np.array_equal(y.cpu().numpy(), want)


def test_degenerate_shapes(env):
    """m = 0 and ncols = 0 write nothing; kdim = 0 writes the bias (ReLU applied), in float32 and in half."""
    L, ops, _ = env
    cen_t = torch.ones(4, device="cuda")
    lab_t = torch.zeros(16, dtype=torch.uint8, device="cuda")
    bias = np.array([-1.5, 2.25, 0.0, 1000.0, -3.0], dtype=np.float32)
    bias_t = torch.from_numpy(bias).cuda()
    for dtype in DTYPES:
        x_t = torch.zeros(8, dtype=_tdt(dtype), device="cuda")
        for half_out in (False, True):
            y, _ = _call(env, x_t, dtype, 3, 0, lab_t, 1, 5, cen_t, 4, bias_t, True, half_out)
            assert np.array_equal(y.cpu().numpy(), np.tile(np.maximum(bias, 0), (3, 1)))
        x2 = torch.zeros((0, 7), dtype=_tdt(dtype), device="cuda")
        assert ops.codebook_matmul(x2, torch.zeros(7 * 5, dtype=torch.uint8, device="cuda"), cen_t, 7, 5).shape == (0, 5)
        assert ops.codebook_matmul(x_t.view(1, 8), torch.zeros(0, dtype=torch.uint8, device="cuda"), cen_t, 8, 0).shape == (1, 0)


# ------------------------------------------------------------------ ops.codebook_matmul
def test_ops_dtype_rules(env):
    _, ops, _ = env
    kdim, ncols, k = 33, 50, 17
    rng = np.random.RandomState(1)
    lab_t = torch.from_numpy(rng.randint(0, k, size=kdim * ncols).astype(np.uint8)).cuda()
    cen_t = torch.from_numpy((rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)).cuda()
    x = torch.from_numpy(rng.randint(-8, 9, size=(2, 20, kdim)).astype(np.float32)).cuda()
    y32 = ops.codebook_matmul(x, lab_t, cen_t, kdim, ncols)
    assert torch.equal(y32, ops.codebook_matmul(x, lab_t, cen_t, kdim, ncols, out_dtype=torch.float32))
    for tdt in (torch.bfloat16, torch.float16):
        yh = ops.codebook_matmul(x.to(tdt), lab_t, cen_t, kdim, ncols)
        assert yh.dtype == tdt and yh.shape == (2, 20, ncols) and torch.equal(yh, y32.to(tdt))
        yf = ops.codebook_matmul(x.to(tdt), lab_t, cen_t, kdim, ncols, out_dtype=torch.float32)
        assert yf.dtype == torch.float32 and torch.equal(yf, y32)
        other = torch.float16 if tdt == torch.bfloat16 else torch.bfloat16
        for bad in (other, torch.float64):
            with pytest.raises(TypeError):
                ops.codebook_matmul(x.to(tdt), lab_t, cen_t, kdim, ncols, out_dtype=bad)
        with pytest.raises(TypeError):
            ops.codebook_matmul(x.to(tdt), lab_t, cen_t.to(tdt), kdim, ncols)
        with pytest.raises(TypeError):
            ops.codebook_matmul(x.to(tdt), lab_t, cen_t, kdim, ncols, bias=torch.zeros(ncols, dtype=tdt, device="cuda"))
        with pytest.raises(TypeError):
            ops.codebook_matmul(x, lab_t, cen_t, kdim, ncols, out_dtype=tdt)
        with pytest.raises(RuntimeError):
            ops.codebook_matmul(x.to(tdt).requires_grad_(), lab_t, cen_t, kdim, ncols)
    with pytest.raises(TypeError):
        ops.codebook_matmul(x.double(), lab_t, cen_t, kdim, ncols)


# ------------------------------------------------------------------ 6. the layers
def _exact_layer_data(rng, kdim, ncols, k):
    lab = rng.randint(0, k, size=kdim * ncols).astype(np.uint8)
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    bias = rng.randint(-50, 51, size=ncols).astype(np.float32)
    return lab, cen, bias


@pytest.mark.parametrize("tdt", [torch.bfloat16, torch.float16])
def test_compressed_dense_on_half_input(env, tdt):
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    kdim, ncols, k = 300, 100, 17
    lab, cen, bias = _exact_layer_data(np.random.RandomState(3), kdim, ncols, k)
    lab_t, cen_t, bias_t = torch.from_numpy(lab).cuda(), torch.from_numpy(cen).cuda(), torch.from_numpy(bias).cuda()
    l1 = compressed.CompressedDense(kdim, ncols, lab_t, cen_t, bias_t, torch.relu)
    l2 = compressed.CompressedDense(ncols, kdim, lab_t, cen_t, None, torch.tanh)
    for m in (1, 5, 40):
        x = torch.randn(m, kdim, device="cuda").to(tdt)
        with torch.no_grad():
            y = l1(x)
            assert y.dtype == tdt and torch.equal(y, ops.codebook_matmul(x, lab_t, cen_t, kdim, ncols, bias=bias_t, relu=True))
            z = l2(y)                                                  # a chain of compressed layers stays in half
            assert z.dtype == tdt and torch.equal(z, torch.tanh(ops.codebook_matmul(y, lab_t, cen_t, ncols, kdim)))
    with torch.no_grad(), pytest.raises(TypeError):                    # a module cast to half: its float32 buffers are gone
        getattr(compressed.CompressedDense(kdim, ncols, lab_t, cen_t, bias_t), "half" if tdt == torch.float16 else "bfloat16")()(x)


@pytest.mark.parametrize("tdt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("ks,cin,cout,pad,hw", [(5, 1, 6, 0, 12), (3, 4, 8, 1, 7)])
def test_compressed_conv_on_half_input(env, monkeypatch, tdt, ks, cin, cout, pad, hw):
    """5 x 5 x 1 -> 6 "valid" and 3 x 3 x 4 -> 8 "same" with exact data: cbmm_ref.conv_nhwc rounded once; a batch that crosses a
    patched-down _PATCH_BYTES (whose chunks count 2-byte elements) gives the same bits; an empty batch an empty result."""
    from neural_network_compression_amd import compressed

    rng = np.random.RandomState(ks)
    k = 17
    lab = rng.randint(0, k, size=ks * ks * cin * cout).astype(np.uint8)
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    bias = rng.randint(-50, 51, size=cout).astype(np.float32)
    layer = compressed.CompressedConv2D.from_codes(ks, cin, cout, pad, torch.from_numpy(lab).cuda(), torch.from_numpy(cen).cuda(),
                                                   torch.from_numpy(bias).cuda(), None)
    n = 5
    x = rng.randint(-8, 9, size=(n, hw, hw, cin)).astype(np.float32)
    want = cbmm_ref.conv_nhwc(x, cen[lab].reshape(ks, ks, cin, cout), pad) + bias.astype(np.float64)
    assert 4 * np.abs(want).max() < 2.0 ** 22
    xt = torch.from_numpy(x).cuda().to(tdt)
    name = "bf16" if tdt == torch.bfloat16 else "fp16"
    with torch.no_grad():
        y = layer(xt)
        assert y.dtype == tdt and y.shape == want.shape
        assert np.array_equal(y.float().cpu().numpy(), round_to(want, name))
        ho = hw + 2 * pad - ks + 1
        calls = []
        orig = layer._matmul
        monkeypatch.setattr(layer, "_matmul", lambda p: (calls.append(p.shape[0]), orig(p))[1])
        monkeypatch.setattr(compressed, "_PATCH_BYTES", 2 * ho * ho * layer.kdim * 2)   # two images of 2-byte patches per chunk
        y2 = layer(xt)
        assert calls == [2, 2, 1] and torch.equal(y, y2)
        calls.clear()
        assert layer(xt.float()).dtype == torch.float32 and calls == [1] * n             # float32 patches: one image per chunk
        e = layer(xt[:0])
        assert e.dtype == tdt and e.shape == (0, ho, ho, cout)


def test_other_forms_raise_type_error_on_half_input(env):
    from neural_network_compression_amd import compressed

    kdim, ncols, k = 64, 32, 9
    lab, cen, bias = _exact_layer_data(np.random.RandomState(8), kdim, ncols, k)
    lab_t, cen_t, bias_t = torch.from_numpy(lab).cuda(), torch.from_numpy(cen).cuda(), torch.from_numpy(bias).cuda()
    layers = [compressed.SparseCompressedDense.from_codes(kdim, ncols, lab_t, cen_t, bias_t, None),
              compressed.PackedCompressedDense.from_codes(kdim, ncols, lab_t, cen_t, bias_t, None),
              compressed.TrainableCompressedDense(kdim, ncols, lab_t, cen_t, bias_t),
              compressed.TrainableSparseCompressedDense.from_codes(kdim, ncols, lab_t, cen_t, bias_t),
              compressed.TrainablePackedCompressedDense.from_codes(kdim, ncols, lab_t, cen_t, bias_t)]
    conv_lab = torch.from_numpy(np.random.RandomState(2).randint(0, k, size=3 * 3 * 2 * 4).astype(np.uint8)).cuda()
    convs = [compressed.SparseCompressedConv2D.from_codes(3, 2, 4, 1, conv_lab, cen_t, None, None),
             compressed.PackedCompressedConv2D.from_codes(3, 2, 4, 1, conv_lab, cen_t, None, None),
             compressed.TrainableCompressedConv2D(3, 2, 4, 1, compressed._unfold_labels(3, 2, 4, conv_lab), cen_t),
             compressed.TrainableSparseCompressedConv2D.from_codes(3, 2, 4, 1, conv_lab, cen_t),
             compressed.TrainablePackedCompressedConv2D.from_codes(3, 2, 4, 1, conv_lab, cen_t)]
    for tdt in (torch.bfloat16, torch.float16):
        for layer in layers:
            with torch.no_grad(), pytest.raises(TypeError, match="byte form"):
                layer(torch.zeros(3, kdim, dtype=tdt, device="cuda"))
            with pytest.raises(TypeError, match="byte form"):
                layer(torch.zeros(3, kdim, dtype=tdt, device="cuda"))
        for layer in convs:
            with torch.no_grad(), pytest.raises(TypeError, match="byte form"):
                layer(torch.zeros(2, 6, 6, 2, dtype=tdt, device="cuda"))


def test_float32_input_keeps_its_bits_through_every_layer(env):
    """float32 input through CompressedDense / CompressedConv2D (and ops.codebook_matmul) is nnc_cbmm_f32 called directly, bit for
    bit, at m on both sides of 16 and with float data."""
    from neural_network_compression_amd import compressed

    L, ops, _ = env
    rng = np.random.RandomState(21)
    kdim, ncols, k = 300, 100, 200
    lab_t = torch.from_numpy(rng.randint(0, k, size=kdim * ncols).astype(np.uint8)).cuda()
    cen_t, bias_t = torch.randn(k, device="cuda"), torch.randn(ncols, device="cuda")

    def direct(x2d, labels, kd, nc, relu):
        m = x2d.shape[0]
        y = torch.empty(m, nc, device="cuda")
        ws_bytes = int(L.nnc_cbmm_workspace_bytes(m, kd, nc, 1))
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device="cuda")
        ops.nat.check(L.nnc_cbmm_f32(x2d.data_ptr(), m, kd, labels.data_ptr(), 1, nc, cen_t.data_ptr(), k, bias_t[:nc].data_ptr(), int(relu),
                                     y.data_ptr(), ws.data_ptr() if ws_bytes else None, ws_bytes, torch.cuda.current_stream().cuda_stream))
        return y

    dense = compressed.CompressedDense(kdim, ncols, lab_t, cen_t, bias_t, torch.relu)
    with torch.no_grad():
        for m in (1, 16, 17, 130):
            x = torch.randn(m, kdim, device="cuda")
            assert torch.equal(dense(x).view(torch.int32), direct(x, lab_t, kdim, ncols, True).view(torch.int32)), m
            assert torch.equal(ops.codebook_matmul(x, lab_t, cen_t, kdim, ncols, bias=bias_t, relu=True).view(torch.int32),
                               direct(x, lab_t, kdim, ncols, True).view(torch.int32)), m
        conv_lab = torch.from_numpy(rng.randint(0, k, size=3 * 3 * 4 * 8).astype(np.uint8)).cuda()
        conv = compressed.CompressedConv2D.from_codes(3, 4, 8, 1, conv_lab, cen_t, bias_t[:8].clone(), None)
        for n in (1, 3):
            x = torch.randn(n, 7, 7, 4, device="cuda")
            patches = compressed.conv_patches(x, 3, 1).contiguous().view(-1, 36)
            assert torch.equal(conv(x).view(-1, 8).view(torch.int32), direct(patches, conv.labels, 36, 8, False).view(torch.int32)), n
