"""The backward pass of the byte-form codebook layers on bfloat16 / float16 activations (nnc_cbmm_dx_h16 / nnc_cbmm_dc_h16,
csrc/nnc_cbgrad_h16.hip), ops.codebook_linear on half x, the trainable layers with half_inputs=True and
Trainer.fine_tune_compressed(activation_dtype=...) (run with -m gpu).

Exact data (integer x and g, dyadic centres) must give the float64 formulas bit for bit in every regime of both plans: every partial
sum is exact, so neither the MFMA's internal order nor the splits can show.  The lane-map tests pin both MFMA kernels' fragment and
accumulator maps.  At m <= 16 the half calls equal the float32 entry points on the widened inputs bit for bit.  Float data stays
within the bounds of section 22 (tests/helpers/h16_grad_ref.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_compression_amd import synth  # noqa: E402
from tests.helpers import cbgrad_ref as ref  # noqa: E402
from tests.helpers import h16_grad_ref as href  # noqa: E402
from tests.helpers import h16_ref  # noqa: E402

TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}
DTYPES = h16_ref.DTYPES


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, ops

    L = _native.load()
    _, cus = ops.device_info()
    return L, ops, cus


def _dev_labels(lab, lb, off):
    """The indices as uint8 / int16 starting ``off`` elements into a buffer with 16 spare bytes of 0xFF after them."""
    dt = torch.uint8 if lb == 1 else torch.int16
    host = lab.astype(np.uint8) if lb == 1 else lab.astype(np.uint16).view(np.int16)
    buf = torch.full((off + host.size + 16 // lb,), -1 if lb == 2 else 255, dtype=dt, device="cuda")
    buf[off: off + host.size] = torch.from_numpy(np.ascontiguousarray(host).ravel()).cuda()
    return buf[off: off + host.size]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _half(a, dtype, view=False):
    """``a`` as a CUDA tensor of ``dtype``; ``view``: as buf[1:] of a buffer one element longer (2 bytes off every wider
    alignment).  Behind the data lie 64 NaNs."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((a.size + 65,), float("nan"), dtype=TDT[dtype], device="cuda")
    lo = 1 if view else 0
    buf[lo: lo + a.size] = torch.from_numpy(a.ravel()).cuda().to(TDT[dtype])
    return buf[lo: lo + a.size].view(a.shape)


def _plans(ops, cus, case, dtype, labels):
    _, m, kdim, ncols, lb, k, _, _ = case[0]
    return (ops.cbmm_dx_h16_plan(TDT[dtype], m, kdim, ncols, lb, k, cus, labels.data_ptr()),
            ops.cbmm_dc_h16_plan(TDT[dtype], m, kdim, ncols, lb, k, cus, labels.data_ptr()))


def test_every_regime_is_covered_at_this_cu_count(env):
    _, ops, cus = env
    dxs, dcs = set(), set()
    for case in href.CASES:
        _, m, kdim, ncols, lb, k, off, _ = case[0]
        lab = _dev_labels(np.zeros((kdim, ncols), dtype=np.int64), lb, off)
        for dtype in DTYPES:
            dxp, dcp = _plans(ops, cus, case, dtype, lab)
            dxs.add(href.regime_of(case, dxp, dtype))
            dcs.add(href.regime_of(case, dcp, dtype))
    assert href.required_regimes("dx") <= dxs and href.required_regimes("dc") <= dcs
    arms = {href.xvec_arms(c) for c in href.FULL if c[0][1] > 16}
    assert {a[0] for a in arms} == {True, False} and {a[1] for a in arms} == {True, False}


# ------------------------------------------------------------------ 1. lane maps
@pytest.mark.parametrize("dtype", DTYPES)
def test_dx_lane_map_identity_g_returns_w_transposed(env, dtype):
    _, ops, _ = env
    m = ncols = 40
    kdim, k = 50, 256
    rng = np.random.RandomState(3)
    c = ((np.arange(k) - 128) / 4.0).astype(np.float32)            # exact in bf16: 127 quarters need 7 bits
    lab = rng.randint(0, k, size=(kdim, ncols))
    w = ref.decoded(lab, c)
    assert not np.array_equal(w[:40, :40], w[:40, :40].T)
    g = _half(np.eye(m), dtype)
    labels, ct = _dev_labels(lab, 1, 0), _cuda(c)
    dx = ops.codebook_matmul_dx(g, labels, ct, kdim, ncols, out_dtype=torch.float32)
    assert np.array_equal(dx.cpu().numpy(), w.T[:m].astype(np.float32))
    dxh = ops.codebook_matmul_dx(g, labels, ct, kdim, ncols)
    assert dxh.dtype == TDT[dtype] and np.array_equal(dxh.float().cpu().numpy(), w.T[:m].astype(np.float32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_dc_lane_map_diagonal_x_returns_every_dw(env, dtype):
    _, ops, _ = env
    kdim, ncols, m, k = 20, 50, 20, 1000
    rng = np.random.RandomState(4)
    lab = np.arange(k).reshape(kdim, ncols)
    x = np.diag(np.arange(1, kdim + 1)).astype(np.float32)         # x[r, i] = delta_ri (i + 1)
    g = rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
    want = (np.arange(1, kdim + 1)[:, None] * g.astype(np.float64)).ravel()
    labels = _dev_labels(lab, 2, 0)
    for out in (torch.float64, torch.float32):
        dc = ops.codebook_centroid_grad(_half(x, dtype), _half(g, dtype), labels, k, kdim, ncols, dtype=out)
        assert np.array_equal(dc.cpu().numpy(), want.astype(dc.cpu().numpy().dtype))


# ------------------------------------------------------------------ 2. exact data, every regime; the same call gives the same bits
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", href.CASES, ids=[href.case_id(c) for c in href.CASES])
def test_exact_data_matches_float64_bit_for_bit(env, case, dtype):
    _, ops, cus = env
    (name, m, kdim, ncols, lb, k, off, _), view = case
    x, g, c, lab = ref.case_data(case[0], seed=len(name) * 5 + m)
    labels, ct = _dev_labels(lab, lb, off), _cuda(c)
    xt, gt = _half(x, dtype, view), _half(g, dtype, view)
    dx = ops.codebook_matmul_dx(gt, labels, ct, kdim, ncols, out_dtype=torch.float32)
    want = ref.dx64(g, lab, c)
    assert dx.shape == (m, kdim) and np.array_equal(dx.cpu().numpy(), want.astype(np.float32))
    dxh = ops.codebook_matmul_dx(gt, labels, ct, kdim, ncols)
    assert dxh.dtype == TDT[dtype] and np.array_equal(dxh.float().cpu().numpy(), h16_ref.round_to(want, dtype))
    assert torch.equal(dx, ops.codebook_matmul_dx(gt, labels, ct, kdim, ncols, out_dtype=torch.float32))
    want_dc = ref.dc64(x, g, lab, k)
    for out in (torch.float64, torch.float32):
        dc = ops.codebook_centroid_grad(xt, gt, labels, k, kdim, ncols, dtype=out)
        assert np.array_equal(dc.cpu().numpy(), want_dc.astype(np.float64 if out == torch.float64 else np.float32)), out
        assert torch.equal(dc, ops.codebook_centroid_grad(xt, gt, labels, k, kdim, ncols, dtype=out))


# ------------------------------------------------------------------ 3. m <= 16 is the float32 entry point on the widened inputs
def _float_data(case, dtype, seed):
    """randn x and g and fitted-layer-like centres (a spread of small values), rounded to ``dtype``; the labels of case_data"""
    _, m, kdim, ncols, lb, k, _, _ = case[0]
    _, _, _, lab = ref.case_data(case[0], seed)
    rng = np.random.RandomState(seed + 1)
    x = h16_ref.round_to(rng.randn(m, kdim), dtype)
    g = h16_ref.round_to(rng.randn(m, ncols) * 0.01, dtype)
    c = (np.sort(rng.randn(k)) * 0.08).astype(np.float32)
    return x, g, c, lab


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in href.FULL if c[0][1] <= 16], ids=href.case_id)
def test_stream_path_equals_the_float32_entry_points(env, case, dtype):
    _, ops, cus = env
    (name, m, kdim, ncols, lb, k, off, _), view = case
    x, g, c, lab = _float_data(case, dtype, seed=m)
    labels, ct = _dev_labels(lab, lb, off), _cuda(c)
    xt, gt = _half(x, dtype, view), _half(g, dtype, view)
    dxp, dcp = _plans(ops, cus, case, dtype, labels)
    f32 = (ops.cbmm_dx_plan(m, kdim, ncols, lb, k, cus, labels.data_ptr()), ops.cbmm_dc_plan(m, kdim, ncols, lb, k, cus, labels.data_ptr()))
    assert all(dxp[f] == v for f, v in f32[0].items()) and all(dcp[f] == v for f, v in f32[1].items())
    dx = ops.codebook_matmul_dx(gt, labels, ct, kdim, ncols, out_dtype=torch.float32)
    assert torch.equal(dx, ops.codebook_matmul_dx(gt.float(), labels, ct.to(TDT[dtype]).float(), kdim, ncols))
    assert torch.equal(ops.codebook_matmul_dx(gt, labels, ct, kdim, ncols), dx.to(TDT[dtype]))
    for out in (torch.float64, torch.float32):
        dc = ops.codebook_centroid_grad(xt, gt, labels, k, kdim, ncols, dtype=out)
        assert torch.equal(dc, ops.codebook_centroid_grad(xt.float(), gt.float(), labels, k, kdim, ncols, dtype=out))


# ------------------------------------------------------------------ 4. float data within the bounds
def _check_bounds(ops, cus, case, dtype, x, g, c, lab):
    """-> the largest err / bound of dx (float32, then half) and dc (float64, then float32)"""
    (name, m, kdim, ncols, lb, k, off, _), view = case
    labels, ct = _dev_labels(lab, lb, off), _cuda(c)
    xt, gt = _half(x, dtype, view), _half(g, dtype, view)
    dxp, dcp = _plans(ops, cus, case, dtype, labels)
    ch = h16_ref.round_to(c, dtype)
    w_h = ref.decoded(lab, ch)
    want = ref.dx64(g, lab, ch)
    bound = href.dx_bound(g, w_h, dxp["splits"]) + 1e-300
    ratios = []
    dx = ops.codebook_matmul_dx(gt, labels, ct, kdim, ncols, out_dtype=torch.float32).double().cpu().numpy()
    ratios.append(np.max(np.abs(dx - want) / bound))
    dxh = ops.codebook_matmul_dx(gt, labels, ct, kdim, ncols).double().cpu().numpy()
    ratios.append(np.max(np.abs(dxh - want) / (bound + h16_ref.half_ulp(want, dtype))))
    S, flag = ops.cbgrad_shift(m, np.abs(x).max(), np.abs(g).max(), dcp["terms_log2"])
    assert flag == ops.CBGRAD_OK
    want_dc = ref.dc64(x, g, lab, k)
    for out in (torch.float64, torch.float32):
        dc = ops.codebook_centroid_grad(xt, gt, labels, k, kdim, ncols, dtype=out).double().cpu().numpy()
        b = href.dc_bound(x, g, lab, k, S, dcp["splits"], f32_out=out == torch.float32) + 1e-300
        ratios.append(np.max(np.abs(dc - want_dc) / b))
    return ratios


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", href.FULL, ids=href.case_id)
def test_float_data_is_within_the_bounds(env, case, dtype):
    _, ops, cus = env
    x, g, c, lab = _float_data(case, dtype, seed=case[0][1] + 11)
    ratios = _check_bounds(ops, cus, case, dtype, x, g, c, lab)
    print(f"err/bound {href.case_id(case)} {dtype}: dx {ratios[0]:.4f} dx_half {ratios[1]:.4f} dc64 {ratios[2]:.4f} dc32 {ratios[3]:.4f}")
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("dtype", DTYPES)
def test_m16_and_m17_agree_within_the_bounds(env, dtype):
    """the stream path at m = 16 and the MFMA path at m = 17 on the same rows: dx row for row, dc up to the last row's terms"""
    _, ops, cus = env
    kdim, ncols, k = 100, 100, 256
    case17 = (("m17", 17, kdim, ncols, 1, k, 0, False), False)
    x, g, c, lab = _float_data(case17, dtype, seed=2)
    labels, ct = _dev_labels(lab, 1, 0), _cuda(c)
    ch = h16_ref.round_to(c, dtype)
    dx17 = ops.codebook_matmul_dx(_half(g, dtype), labels, ct, kdim, ncols, out_dtype=torch.float32).double().cpu().numpy()
    dx16 = ops.codebook_matmul_dx(_half(g[:16], dtype), labels, ct, kdim, ncols, out_dtype=torch.float32).double().cpu().numpy()
    b = href.dx_bound(g[:16], ref.decoded(lab, ch), 1)
    assert np.all(np.abs(dx17[:16] - dx16) <= 2 * b)
    dc17 = ops.codebook_centroid_grad(_half(x, dtype), _half(g, dtype), labels, k, kdim, ncols).cpu().numpy()
    dc16 = ops.codebook_centroid_grad(_half(x[:16], dtype), _half(g[:16], dtype), labels, k, kdim, ncols).cpu().numpy()
    last = ref.dc64(x[16:], g[16:], lab, k)
    T = ops.cbmm_dc_h16_plan(TDT[dtype], 17, kdim, ncols, 1, k, cus)["terms_log2"]
    S = min(ops.cbgrad_shift(mm, np.abs(x[:mm]).max(), np.abs(g[:mm]).max(), T)[0] for mm in (16, 17))
    b = href.dc_bound(x, g, lab, k, S, 1) + href.dc_bound(x[:16], g[:16], lab, k, S, 1)
    assert np.all(np.abs(dc17 - dc16 - last) <= b)


# ------------------------------------------------------------------ 5. memory safety
F16_SENTINEL = 0x7BCD


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in href.FULL if c[0][0] in ("stream_m9_u8_split", "mfma_m130_u8_msplit", "mfma_m256_u16_views")],
                         ids=href.case_id)
def test_nothing_is_written_or_read_out_of_bounds(env, case, dtype):
    """sentinel frames around dx (2-byte granularity for a half dx), dc and the workspace; NaNs directly behind x and g and 0xFF bytes
    behind the labels (the helpers put them there) do not reach a result"""
    from neural_network_compression_amd import _native as nat

    L, ops, cus = env
    (name, m, kdim, ncols, lb, k, off, _), view = case
    x, g, c, lab = ref.case_data(case[0], seed=7)
    labels, ct = _dev_labels(lab, lb, off), _cuda(c)
    xt, gt = _half(x, dtype, view), _half(g, dtype, view)
    dt = h16_ref.DT_CODE[dtype]
    stream = torch.cuda.current_stream().cuda_stream
    PAD = 64
    for out_dt in (0, dt):
        esz = 4 if out_dt == 0 else 2
        frame = torch.full((2 * PAD + m * kdim * esz // 2,), F16_SENTINEL, dtype=torch.int16, device="cuda")
        ws_bytes = int(L.nnc_cbmm_dx_h16_workspace_bytes(m, kdim, ncols, lb))
        ws = torch.full((ws_bytes + 2 * PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        dx_ptr = frame.data_ptr() + 2 * PAD
        nat.check(L.nnc_cbmm_dx_h16(gt.data_ptr(), dt, m, kdim, labels.data_ptr(), lb, ncols, ct.data_ptr(), k, dx_ptr, out_dt,
                                    ws.data_ptr() + PAD, ws_bytes, stream))
        torch.cuda.synchronize()
        assert (frame[:PAD] == F16_SENTINEL).all() and (frame[-PAD:] == F16_SENTINEL).all()
        assert (ws[:PAD] == 0xA5).all() and (ws[-PAD:] == 0xA5).all()
        body = frame[PAD:-PAD]
        got = body.view(torch.float32) if out_dt == 0 else body.view(TDT[dtype]).float()
        want = ref.dx64(g, lab, c)
        assert np.array_equal(got.cpu().numpy().reshape(m, kdim), want.astype(np.float32) if out_dt == 0 else h16_ref.round_to(want, dtype))
    for f64 in (1, 0):
        sent = -7.25
        frame = torch.full((2 * PAD + k,), sent, dtype=torch.float64 if f64 else torch.float32, device="cuda")
        ws_bytes = int(L.nnc_cbmm_dc_h16_workspace_bytes(m, kdim, ncols, lb, k))
        ws = torch.full((ws_bytes + 2 * PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        nat.check(L.nnc_cbmm_dc_h16(xt.data_ptr(), gt.data_ptr(), dt, m, kdim, labels.data_ptr(), lb, ncols, k,
                                    frame.data_ptr() + PAD * frame.element_size(), f64, ws.data_ptr() + PAD, ws_bytes, stream))
        torch.cuda.synchronize()
        assert (frame[:PAD] == sent).all() and (frame[-PAD:] == sent).all()
        assert (ws[:PAD] == 0xA5).all() and (ws[-PAD:] == 0xA5).all()
        want = ref.dc64(x, g, lab, k)
        assert np.array_equal(frame[PAD:-PAD].cpu().numpy(), want if f64 else want.astype(np.float32))


# ------------------------------------------------------------------ 6. range
RANGE_CASES = [c for c in href.FULL if c[0][0] in ("stream_m5_u16_k257", "mfma_m40_u16_dxsplit")]


def _f32(a):
    with np.errstate(over="ignore", under="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float32)


@pytest.mark.parametrize("case", RANGE_CASES, ids=href.case_id)
def test_bf16_dc_across_the_exponent_range(env, case):
    """exact data scaled far down (x 2^-100, g 2^-60) and near the top on both sides of P = 127: dc is still the float64 formula,
    or all NaN beyond P = 127"""
    _, ops, cus = env
    (name, m, kdim, ncols, lb, k, off, _), view = case
    x, g, c, lab = ref.case_data(case[0], seed=13)
    x[0, 0] = g[0, 0] = 3.0
    labels = _dev_labels(lab, lb, off)
    T = ops.cbmm_dc_h16_plan(torch.bfloat16, m, kdim, ncols, lb, k, cus)["terms_log2"]
    for ex, eg, finite in ((-100, -60, True), (58, 58, True), (61, 62 - int(np.ceil(np.log2(m))), None), (62, 62, False)):
        xs, gs = np.ldexp(x, ex), np.ldexp(g, eg)
        S, flag = ops.cbgrad_shift(m, 3.0 * 2.0 ** ex, 3.0 * 2.0 ** eg, T)
        if finite is None:                               # the third: the last exponents with P <= 127, by the mirror
            assert flag == ops.CBGRAD_OK and ops.cbgrad_shift(m, 3.0 * 2.0 ** (ex + 1), 3.0 * 2.0 ** (eg + 1), T)[1] == ops.CBGRAD_NONFINITE
        else:
            assert (flag == ops.CBGRAD_OK) == finite
        want = np.ldexp(ref.dc64(x, g, lab, k), ex + eg)
        for out in (torch.float64, torch.float32):
            dc = ops.codebook_centroid_grad(_half(xs, "bf16"), _half(gs, "bf16"), labels, k, kdim, ncols, dtype=out).cpu().numpy()
            if flag == ops.CBGRAD_OK:
                assert np.array_equal(dc, want if out == torch.float64 else _f32(want)), (ex, eg, out)
            else:
                assert np.isnan(dc).all()


@pytest.mark.parametrize("case", RANGE_CASES, ids=href.case_id)
def test_fp16_dc_with_the_largest_value_next_to_subnormals(env, case):
    """x[0, 0] = 65504 in a column that is otherwise 0, every other x a subnormal 2^-24 {0..3}: every dW is exact in float32 and,
    with S >= 24 (asserted), so is its fixed-point image: dc is the float64 formula although nothing is scaled"""
    _, ops, cus = env
    (name, m, kdim, ncols, lb, k, off, _), view = case
    x, g, c, lab = ref.case_data(case[0], seed=17)
    x = np.abs(x) * 2.0 ** -24
    x[:, 0] = 0.0
    x[0, 0] = 65504.0
    g[0, 0] = 3.0
    labels = _dev_labels(lab, lb, off)
    T = ops.cbmm_dc_h16_plan(torch.float16, m, kdim, ncols, lb, k, cus)["terms_log2"]
    S, flag = ops.cbgrad_shift(m, 65504.0, 3.0, T)
    assert flag == ops.CBGRAD_OK and S >= 24
    want = ref.dc64(x, g, lab, k)
    for out in (torch.float64, torch.float32):
        dc = ops.codebook_centroid_grad(_half(x, "fp16"), _half(g, "fp16"), labels, k, kdim, ncols, dtype=out).cpu().numpy()
        assert np.array_equal(dc, want if out == torch.float64 else _f32(want))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", RANGE_CASES, ids=href.case_id)
def test_non_finite_inputs(env, case, dtype):
    _, ops, cus = env
    (name, m, kdim, ncols, lb, k, off, _), view = case
    x, g, c, lab = ref.case_data(case[0], seed=19)
    labels, ct = _dev_labels(lab, lb, off), _cuda(c)
    for bad in (np.nan, np.inf):
        gb = g.copy()
        gb[1, 5] = bad
        xb = x.copy()
        xb[2, 3] = bad
        for xx, gg in ((xb, g), (x, gb)):
            dc = ops.codebook_centroid_grad(_half(xx, dtype), _half(gg, dtype), labels, k, kdim, ncols).cpu().numpy()
            assert np.isnan(dc).all()
        dx = ops.codebook_matmul_dx(_half(gb, dtype), labels, ct, kdim, ncols, out_dtype=torch.float32).cpu().numpy()
        with np.errstate(invalid="ignore"):
            want = ref.dx64(gb, lab, c).astype(np.float32)
        assert np.array_equal(dx, want, equal_nan=True) and not np.isfinite(dx[1]).any() and np.isfinite(np.delete(dx, 1, axis=0)).all()


def test_an_fp16_centre_beyond_the_range_acts_as_inf_in_dx(env):
    _, ops, _ = env
    case = RANGE_CASES[1][0]
    _, m, kdim, ncols, lb, k, off, _ = case
    x, g, c, lab = ref.case_data(case, seed=23)
    c[7] = 1e5
    ch = c.astype(np.float64)
    ch[7] = np.inf
    with np.errstate(invalid="ignore"):
        want = ref.dx64(g, lab, ch).astype(np.float32)
    dx = ops.codebook_matmul_dx(_half(g, "fp16"), _dev_labels(lab, lb, off), _cuda(c), kdim, ncols, out_dtype=torch.float32).cpu().numpy()
    assert not np.isfinite(want).all() and np.array_equal(dx, want, equal_nan=True)


# ------------------------------------------------------------------ 7. ops.codebook_linear on half x
def _exact_layer(m=6, kdim=90, ncols=150, k=40, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.randint(-3, 4, size=(m, kdim)).astype(np.float32)
    c = (rng.randint(-8, 9, size=k) / 4.0).astype(np.float32)
    lab = rng.randint(0, k, size=(kdim, ncols))
    b = rng.randint(-5, 6, size=ncols).astype(np.float32)
    return x, c, lab, b


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [5, 40])
@pytest.mark.parametrize("relu", [False, True])
def test_codebook_linear_on_half_x_is_the_direct_calls(env, m, relu, dtype):
    _, ops, _ = env
    x, c, lab, b = _exact_layer(m=m, seed=m)
    gy = np.random.RandomState(m + 1).randn(m, 150).astype(np.float32)
    xt = _half(x * 0.37, dtype).requires_grad_(True)
    ct, bt, labels = _cuda(c).requires_grad_(True), _cuda(b).requires_grad_(True), _dev_labels(lab, 1, 1)
    y = ops.codebook_linear(xt, labels, ct, 90, 150, bias=bt, relu=relu)
    with torch.no_grad():
        want = ops.codebook_matmul(xt, labels, ct, 90, 150, bias=bt, relu=relu)
    assert y.dtype == TDT[dtype] and torch.equal(y, want)
    gt = _half(gy, dtype)
    y.backward(gt)
    g = torch.where(want > 0, gt, torch.zeros((), dtype=gt.dtype, device="cuda")) if relu else gt
    assert xt.grad.dtype == TDT[dtype] and torch.equal(xt.grad, ops.codebook_matmul_dx(g, labels, ct.detach(), 90, 150))
    assert ct.grad.dtype == torch.float32
    assert torch.equal(ct.grad, ops.codebook_centroid_grad(xt.detach(), g, labels, 40, 90, 150, dtype=torch.float32))
    assert bt.grad.dtype == torch.float32 and torch.equal(bt.grad, g.float().sum(0))


@pytest.mark.parametrize("dtype", DTYPES)
def test_relu_gives_nan_and_negative_outputs_a_zero_gradient(env, dtype):
    _, ops, _ = env
    x, c, lab, b = _exact_layer(m=4, seed=9)
    x[0, 3] = np.nan                                          # row 0 of y is NaN
    xt, ct = _half(x, dtype).requires_grad_(True), _cuda(c)
    labels = _dev_labels(lab, 1, 0)
    y = ops.codebook_linear(xt, labels, ct, 90, 150, relu=True)
    yh = y.detach().float().cpu().numpy()
    assert np.isnan(yh[0]).all() and (yh[1:] == 0).any()
    y.backward(torch.ones_like(y))
    mask = np.where(np.nan_to_num(yh, nan=-1.0) > 0, 1.0, 0.0)
    got = xt.grad.float().cpu().numpy()
    assert (got[0] == 0).all()
    assert np.array_equal(got, h16_ref.round_to(ref.dx64(mask, lab, c), dtype))


def test_only_the_needed_kernels_run(env, monkeypatch):
    _, ops, _ = env
    x, c, lab, b = _exact_layer(m=3)
    labels = _dev_labels(lab, 1, 0)
    calls = []
    real_dx, real_dc = ops.codebook_matmul_dx, ops.codebook_centroid_grad
    monkeypatch.setattr(ops, "codebook_matmul_dx", lambda *a, **k: calls.append("dx") or real_dx(*a, **k))
    monkeypatch.setattr(ops, "codebook_centroid_grad", lambda *a, **k: calls.append("dc") or real_dc(*a, **k))
    ops.codebook_linear(_half(x, "bf16").requires_grad_(True), labels, _cuda(c), 90, 150).float().sum().backward()
    assert calls == ["dx"]
    calls.clear()
    ops.codebook_linear(_half(x, "bf16"), labels, _cuda(c).requires_grad_(True), 90, 150).float().sum().backward()
    assert calls == ["dc"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_and_backward_read_nothing_back(env, dtype):
    _, ops, _ = env
    x, c, lab, b = _exact_layer(m=16)
    xt, ct, bt = _half(x, dtype).requires_grad_(True), _cuda(c).requires_grad_(True), _cuda(b).requires_grad_(True)
    x40 = _half(np.tile(x[:5], (8, 1)), dtype).requires_grad_(True)
    labels = _dev_labels(lab, 1, 0)
    gy, gy40 = torch.ones(16, 150, device="cuda", dtype=TDT[dtype]), torch.ones(40, 150, device="cuda", dtype=TDT[dtype])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for relu in (False, True):
            ops.codebook_linear(xt, labels, ct, 90, 150, bias=bt, relu=relu).backward(gy)
            ops.codebook_linear(x40, labels, ct, 90, 150, relu=relu).backward(gy40)
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_dtype_errors(env):
    _, ops, _ = env
    x, c, lab, b = _exact_layer(m=3)
    labels, ct, bt = _dev_labels(lab, 1, 0), _cuda(c), _cuda(b)
    g = _half(np.ones((3, 150)), "bf16")
    xh = _half(x, "bf16")
    with pytest.raises(TypeError):
        ops.codebook_matmul_dx(g, labels, ct.bfloat16(), 90, 150)
    with pytest.raises(TypeError):
        ops.codebook_matmul_dx(g, labels, ct, 90, 150, out_dtype=torch.float16)
    with pytest.raises(TypeError):
        ops.codebook_matmul_dx(g.float(), labels, ct, 90, 150, out_dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        ops.codebook_centroid_grad(xh, g.half(), labels, 40, 90, 150)
    with pytest.raises(TypeError):
        ops.codebook_centroid_grad(xh.float(), g, labels, 40, 90, 150)
    with pytest.raises(TypeError):
        ops.codebook_linear(xh, labels, ct.bfloat16(), 90, 150)
    with pytest.raises(TypeError):
        ops.codebook_linear(xh, labels, ct, 90, 150, bias=bt.bfloat16())


# ------------------------------------------------------------------ 8. the layers
@pytest.mark.parametrize("dtype", DTYPES)
def test_trainable_dense_with_half_inputs(env, dtype):
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    x, c, lab, b = _exact_layer(m=40, seed=2)
    labels, ct, bt = _dev_labels(lab, 1, 0), _cuda(c), _cuda(b)
    layer = compressed.TrainableCompressedDense(90, 150, labels, ct, bt, None, torch.relu, half_inputs=True)
    xt = _half(x, dtype).requires_grad_(True)
    y = layer(xt)
    with torch.no_grad():
        want = ops.codebook_matmul(xt, labels, ct, 90, 150, bias=bt, relu=True)
    assert y.dtype == TDT[dtype] and torch.equal(y, want)
    gt = _half(np.random.RandomState(1).randint(-3, 4, size=(40, 150)), dtype)
    y.backward(gt)
    g = torch.where(want > 0, gt, torch.zeros((), dtype=gt.dtype, device="cuda"))
    assert torch.equal(layer.centers.grad, ops.codebook_centroid_grad(xt.detach(), g, labels, 40, 90, 150, dtype=torch.float32))
    assert torch.equal(xt.grad, ops.codebook_matmul_dx(g, labels, ct, 90, 150))
    plain = compressed.TrainableCompressedDense(90, 150, labels, ct, bt, None, torch.relu)
    with pytest.raises(TypeError, match="half_inputs"):
        plain(xt.detach())
    with pytest.raises(TypeError, match="byte form"):
        plain(xt.detach())
    assert plain(xt.detach().float()).dtype == torch.float32 and layer(xt.detach().float()).dtype == torch.float32


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ks,cin,cout,pad,hw", [(5, 1, 6, 0, 12), (3, 4, 8, 1, 7)])
def test_trainable_conv_with_half_inputs(env, dtype, ks, cin, cout, pad, hw):
    """exact data: the layer's output and centre gradient are the ops calls on the patches, which are the float64 formulas"""
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    rng = np.random.RandomState(ks)
    k, kdim = 9, ks * ks * cin
    lab = rng.randint(0, k, size=kdim * cout).astype(np.uint8)
    c = (rng.randint(-4, 5, size=k) / 4.0).astype(np.float32)
    lab_u = compressed._unfold_labels(ks, cin, cout, _cuda(lab))
    layer = compressed.TrainableCompressedConv2D(ks, cin, cout, pad, lab_u, _cuda(c), None, None, None, half_inputs=True)
    x = rng.randint(-2, 3, size=(3, hw, hw, cin)).astype(np.float32)
    xt = _half(x, dtype).requires_grad_(True)
    y = layer(xt)
    ho = hw + 2 * pad - ks + 1
    assert y.dtype == TDT[dtype] and y.shape == (3, ho, ho, cout)
    patches = compressed.conv_patches(xt.detach(), ks, pad).contiguous().reshape(-1, kdim)
    lab2d = lab_u.cpu().numpy().reshape(kdim, cout)
    p64 = patches.double().cpu().numpy()
    assert np.array_equal(y.detach().float().cpu().numpy().reshape(-1, cout), h16_ref.round_to(p64 @ ref.decoded(lab2d, c), dtype))
    gy = rng.randint(-2, 3, size=tuple(y.shape)).astype(np.float32)
    y.backward(_half(gy, dtype))
    want = ref.dc64(p64, gy.reshape(-1, cout), lab2d, k)
    assert np.array_equal(layer.centers.grad.cpu().numpy(), want.astype(np.float32))
    assert xt.grad.dtype == TDT[dtype] and xt.grad.shape == xt.shape
    with pytest.raises(TypeError, match="half_inputs"):
        compressed.TrainableCompressedConv2D(ks, cin, cout, pad, lab_u, _cuda(c))(xt.detach())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [5, 40])
def test_two_layer_chain_with_exact_data_is_float64_autograd(env, m, dtype):
    """20 -> 24 -> 10 with x in {-1, 0, 1} (4 non-zeros a row), first centres multiples of 1/2 in [-1, 1], second in {-1, 0, 1},
    upstream gradient in {-1, 0, 1}: every intermediate is exact in the dtype (asserted in float64), so all centre gradients equal
    float64 autograd on the decoded weights bit for bit"""
    from neural_network_compression_amd import compressed

    rng = np.random.RandomState(m)
    x = np.zeros((m, 20))
    for r in range(m):
        x[r, rng.choice(20, 4, replace=False)] = rng.choice([-1.0, 1.0], 4)
    c1, c2 = np.array([-1, -0.5, 0, 0.5, 1], dtype=np.float32), np.array([-1, 0, 1], dtype=np.float32)
    lab1, lab2 = rng.randint(0, 5, size=(20, 24)), rng.randint(0, 3, size=(24, 10))
    gy = rng.randint(-1, 2, size=(m, 10)).astype(np.float64)
    w1, w2 = torch.from_numpy(ref.decoded(lab1, c1)).requires_grad_(True), torch.from_numpy(ref.decoded(lab2, c2)).requires_grad_(True)
    h = torch.from_numpy(x) @ w1
    h.retain_grad()
    y = h @ w2
    y.backward(torch.from_numpy(gy))
    for t in (h.detach(), y.detach(), h.grad):                 # the precondition: exact in the dtype
        assert np.array_equal(h16_ref.round_to(t.numpy(), dtype), t.numpy())
    l1 = compressed.TrainableCompressedDense(20, 24, _dev_labels(lab1, 1, 0), _cuda(c1), half_inputs=True)
    l2 = compressed.TrainableCompressedDense(24, 10, _dev_labels(lab2, 1, 0), _cuda(c2), half_inputs=True)
    out = l2(l1(_half(x, dtype)))
    assert np.array_equal(out.detach().float().cpu().numpy(), y.detach().numpy())
    out.backward(_half(gy, dtype))
    for layer, w, lab, k in ((l1, w1, lab1, 5), (l2, w2, lab2, 3)):
        want = ref.bin64(w.grad.numpy(), lab, k)
        assert np.array_equal(layer.centers.grad.cpu().numpy(), want.astype(np.float32))


# ------------------------------------------------------------------ 9. the trainer
def _lenet300(seed=0):
    from neural_network_compression_amd import le_net_300_100_trainer as lt
    from neural_network_compression_amd.common import trainer as tr

    tr.Trainer.pruned_indexes_by_layer.clear()
    torch.manual_seed(seed)
    t = lt.LeNet300100Trainer()
    for li, (name, wshape, bshape) in enumerate(synth.LENET_300_100):
        layer = getattr(t.neural_network, name)
        layer.set_weights([torch.from_numpy(synth.weights(wshape, 2000 + 2 * li)).cuda(), torch.from_numpy(synth.weights(bshape, 2001 + 2 * li)).cuda()])
    return t, tr


@pytest.fixture(scope="module")
def quantized(env):
    t, tr = _lenet300()
    rng = np.random.RandomState(1)
    x = rng.rand(512, 784).astype(np.float32)
    y = np.eye(10, dtype=np.float32)[rng.randint(0, 10, size=512)]
    test = tr.LeNetDataset(x[:256], y[:256].argmax(1))
    t.quantize(test, False, 4, "linear")
    return t, tr, tr.LeNetDataset(x, y), test


def _centres(models):
    return {(layer, ti): m.cluster_centers_.ravel().copy() for layer, ms in models.items() for ti, m in enumerate(ms) if m is not None}


def test_one_batch_of_fine_tune_compressed_in_bf16_is_the_step_from_the_ops_calls(env, quantized):
    _, ops, _ = env
    t, tr, data, test = quantized
    models = t.quantized_models_by_layer
    dt, lr = torch.bfloat16, 1e-2
    c0 = _centres(models)
    names = ("dense1", "dense2", "out")
    layers = [getattr(t.neural_network, n) for n in names]
    # the step from the ops calls, on the batch fine_tune_compressed will draw
    torch.manual_seed(5)
    xb, yb = next(tr._batches(t._to_device(data.input_data).float(), t._to_device(data.output_data).float()))
    cs = [torch.from_numpy(c0[(l, 0)]).cuda() for l in layers]
    bcs = [torch.from_numpy(c0[(l, 1)]).cuda() if (l, 1) in c0 else None for l in layers]   # (a bias too short to quantize stays raw)
    assert any(b is not None for b in bcs)
    labs = [models[l][0].labels_compact_ for l in layers]
    blabs = [models[l][1].labels_compact_ if (l, 1) in c0 else None for l in layers]
    biases = [ops.gather(bcs[i], blabs[i]) if bcs[i] is not None else layers[i].bias.detach() for i in range(3)]
    shapes = [tuple(l.kernel.shape) for l in layers]
    acts = [xb.to(dt)]
    with torch.no_grad():
        for i in range(3):
            acts.append(ops.codebook_matmul(acts[-1], labs[i], cs[i], *shapes[i], bias=biases[i], relu=i < 2))
    logits = acts[-1].float().requires_grad_(True)
    torch.nn.functional.binary_cross_entropy_with_logits(logits, yb).backward()
    g = logits.grad.to(dt)
    want = {}
    for i in (2, 1, 0):
        if i < 2:
            g = torch.where(acts[i + 1] > 0, g, torch.zeros((), dtype=dt, device="cuda"))
        dc = ops.codebook_centroid_grad(acts[i], g, labs[i], cs[i].numel(), *shapes[i], dtype=torch.float32)
        cp = cs[i].clone().requires_grad_(True)
        counts = ops.bincount(labs[i], cs[i].numel())
        (0.01 * ((counts.to(torch.float32) * cp ** 2).sum() / 2)).backward()
        want[(layers[i], 0)] = (cs[i], dc, cp.grad)
        if bcs[i] is not None:
            db = ops.centroid_gradient(g.sum(0, dtype=torch.float32).contiguous(), blabs[i], bcs[i].numel()).to(torch.float32)
            want[(layers[i], 1)] = (bcs[i], db, None)
        if i > 0:
            g = ops.codebook_matmul_dx(g, labs[i], cs[i], *shapes[i])

    torch.manual_seed(5)
    t.fine_tune_compressed(data, test, epochs=1, learning_rate=0.0, activation_dtype=dt)
    assert all(np.array_equal(c, c0[key]) for key, c in _centres(models).items())      # learning_rate = 0: bit-identical
    torch.manual_seed(5)
    t.fine_tune_compressed(data, test, epochs=1, learning_rate=lr, activation_dtype=dt)
    got = _centres(models)                                                               # the tuned centres reached the models
    for key, (c, grad, l2) in want.items():
        steps = [c - lr * (grad + l2), c - lr * (l2 + grad)] if l2 is not None else [c - lr * grad]
        assert any(np.array_equal(got[key], s.cpu().numpy()) for s in steps), key
        assert not np.array_equal(got[key], c0[key])
    for layer in layers:                                                                 # and the float layers are re-decoded
        assert torch.equal(layer.kernel.detach().reshape(-1), ops.gather(torch.from_numpy(got[(layer, 0)]).cuda(), models[layer][0].labels_compact_))


def test_fine_tune_compressed_activation_dtype_errors(env, quantized):
    t, tr, data, test = quantized
    for kw in (dict(sparse=True), dict(sparse="auto"), dict(packed=True), dict(packed="auto")):
        with pytest.raises(ValueError):
            t.fine_tune_compressed(data, test, epochs=1, activation_dtype=torch.bfloat16, **kw)
    with pytest.raises(ValueError):
        t.fine_tune_compressed(data, test, epochs=1, activation_dtype=torch.float64)
    with pytest.raises(ValueError):
        t.compressed_network(trainable=True, half_inputs=True, sparse=True)
    with pytest.raises(ValueError):
        t.compressed_network(half_inputs=True)
    net = t.compressed_network(trainable=True, half_inputs=True)
    assert all(layer.half_inputs for layer in net.get_config().values())
    models = t.quantized_models_by_layer
    kept = models[t.neural_network.dense2]
    models[t.neural_network.dense2] = [None, None]              # dense2 passed through unquantized
    try:
        with pytest.raises(ValueError, match="dense2"):
            t.fine_tune_compressed(data, test, epochs=1, activation_dtype=torch.float16)
    finally:
        models[t.neural_network.dense2] = kept
