"""The backward pass of the 2- / 4-bit packed codebook layer on bf16 / fp16 activations (nnc_cbpk_dx_h16 / nnc_cbpk_dc_h16,
csrc/nnc_cbpk_h16.hip), through the raw C ABI with buffers the test owns, through ops.packed_codebook_* and
ops.packed_codebook_linear, through the trainable packed layers built with half_inputs=True and through
Trainer.fine_tune_compressed(packed=..., activation_dtype=..., packed_half_inputs=True) (run with -m gpu).

What it is held to needs no tolerance but the float-data bound.  dc equals ops.codebook_centroid_grad on the unpacked labels and the
same half inputs bit for bit at every m.  Above 16 rows dx equals ops.codebook_matmul_dx on the unpacked labels bit for bit; up to 16
rows the float32 dx is ops.packed_codebook_matmul_dx on the widened g and the rounded centres bit for bit and a half dx is that value
rounded once.  On exact data (integer x and g in [-3, 3], centres multiples of 1/4 in [-2, 2]: every partial sum is exact in float32
in any order) all of them equal the float64 formulas.  Every raw call writes into sentinel-framed outputs and workspace, reads x and g
directly in front of NaN bit patterns and the packed rows at the very end of their tensor, and is repeated for the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_compression_amd import synth  # noqa: E402
from tests.helpers import cbgrad_ref as ref  # noqa: E402
from tests.helpers import h16_grad_ref as href  # noqa: E402
from tests.helpers import h16_ref  # noqa: E402
from tests.helpers import packed_h16_ref as pref  # noqa: E402
from tests.helpers.h16_ref import DTYPES, round_to  # noqa: E402
from tests.helpers.packed_h16_ref import CASES, FULL  # noqa: E402

SENT16 = 0x7FA5              # as bf16 and as fp16 a NaN whose payload neither the inputs nor the kernels' own NaNs carry
SENT32 = 0x7FA57FA5
SENT64 = 0x7FA57FA57FA57FA5
WS_PAD = 64
WORST = {"dx": 0.0, "dc": 0.0}   # the largest err / bound seen on float data (printed by the last test of the file)


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
    """host values -> a device tensor of the dtype that ends directly in front of NaN bit patterns (0xFFFF units); ``view``: it starts
    one element into its buffer (aligned to the element size and no further)."""
    t = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).to(_tdt(dtype))
    off = 1 if view else 0
    buf = torch.full((off + t.numel() + 64,), -1, dtype=torch.int16, device="cuda")
    x = buf[off: off + t.numel()].view(_tdt(dtype))
    x.copy_(t.reshape(-1))
    return x.view(t.shape)


def _dev_labels(lab):
    return _cuda(np.ascontiguousarray(lab, dtype=np.uint8).ravel())


def _codes(env, lab, bits, k):
    """The packed form of lab (kdim, ncols), moved so that its last row ends with its tensor (256 bytes of 0xFF in front keep the
    alignment)."""
    _, ops, _ = env
    kdim, ncols = lab.shape
    codes = ops.pack_codes(_dev_labels(lab), kdim, ncols, k, bits)
    big = torch.full((256 + codes.nbytes,), 255, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 256 == 0
    big[256:] = codes.packed
    return ops.PackedCodes(big[256:], kdim, ncols, bits, k)


def _framed(units, pad, sent, tdtype):
    buf = torch.full((units + 2 * pad,), sent, dtype=tdtype, device="cuda")
    return buf, buf[pad: pad + units]


def _raw_dx(env, g, dtype, codes, centers, half_out):
    """nnc_cbpk_dx_h16 into sentinel-framed dx and workspace (exactly the queried size); checks the frames; returns dx (m, kdim)."""
    L, ops, _ = env
    m, kdim, ncols, bits = g.shape[0], codes.kdim, codes.ncols, codes.bits
    ws_bytes = int(L.nnc_cbpk_dx_h16_workspace_bytes(m, kdim, ncols, bits))
    assert ws_bytes % 4 == 0
    units, pad = (m * kdim, 37) if half_out else (2 * m * kdim, 38)
    obuf, out = _framed(units, pad, SENT16, torch.int16)
    wbuf, ws = _framed(ws_bytes // 4, WS_PAD, SENT32, torch.int32)
    dt = h16_ref.DT_CODE[dtype]
    ops.nat.check(L.nnc_cbpk_dx_h16(g.data_ptr(), dt, m, kdim, codes.packed.data_ptr(), codes.nbytes, bits, ncols, centers.data_ptr(), centers.numel(),
                                    out.data_ptr(), dt if half_out else 0, ws.data_ptr() if ws_bytes else None, ws_bytes,
                                    torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((obuf[:pad] == SENT16).all()) and bool((obuf[pad + units:] == SENT16).all()), "a store outside dx"
    assert bool((wbuf[:WS_PAD] == SENT32).all()) and bool((wbuf[WS_PAD + ws_bytes // 4:] == SENT32).all()), "a store outside the workspace"
    if half_out:
        assert not bool((out == SENT16).any()), "an output left unwritten"
        return out.clone().view(_tdt(dtype)).view(m, kdim)
    assert not bool((out.view(torch.int32) == SENT32).any()), "an output left unwritten"
    return out.clone().view(torch.float32).view(m, kdim)


def _raw_dc(env, x, g, dtype, codes, f64):
    """nnc_cbpk_dc_h16 into sentinel-framed dc and workspace; checks the frames; returns dc [k]."""
    L, ops, _ = env
    m, kdim, ncols, bits, k = x.shape[0], codes.kdim, codes.ncols, codes.bits, codes.k
    ws_bytes = int(L.nnc_cbpk_dc_h16_workspace_bytes(m, kdim, ncols, bits, k))
    assert ws_bytes == 64 + 8 * k
    sent = SENT64 if f64 else SENT32
    obuf, out = _framed(k, 8, sent, torch.int64 if f64 else torch.int32)
    wbuf, ws = _framed(ws_bytes // 8, WS_PAD, SENT64, torch.int64)
    ops.nat.check(L.nnc_cbpk_dc_h16(x.data_ptr(), g.data_ptr(), h16_ref.DT_CODE[dtype], m, kdim, codes.packed.data_ptr(), codes.nbytes, bits, ncols, k,
                                    out.data_ptr(), 1 if f64 else 0, ws.data_ptr(), ws_bytes, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((obuf[:8] == sent).all()) and bool((obuf[8 + k:] == sent).all()), "a store outside dc"
    assert bool((wbuf[:WS_PAD] == SENT64).all()) and bool((wbuf[WS_PAD + ws_bytes // 8:] == SENT64).all()), "a store outside the workspace"
    assert not bool((out == sent).any()), "a bin left unwritten"
    return out.clone().view(torch.float64 if f64 else torch.float32)


def _case_setup(env, case, dtype, data):
    """(x, g, centres, labels (kdim, ncols), codes, x_t, g_t, c_t, dense labels tensor) of a case: exact or float data, rounded to dtype"""
    (_, m, kdim, ncols, bits, k, _, _), view = case
    x, g, cen, lab = pref.case_data(case[0], 17 + m + 3 * kdim + 5 * ncols)
    if data == "float":   # h16_grad_ref's recipe
        rng = np.random.RandomState(17 + m + 3 * kdim + 5 * ncols)
        x = round_to(rng.randn(m, kdim), dtype)
        g = round_to(rng.randn(m, ncols) * 0.01, dtype)
        cen = (np.sort(rng.randn(k)) * 0.08).astype(np.float32)
    return x, g, cen, lab, _codes(env, lab, bits, k), _half(x, dtype, view), _half(g, dtype, view), _cuda(cen), _dev_labels(lab)


def test_every_regime_is_covered_at_this_cu_count(env):
    _, ops, cus = env
    dxs, dcs = set(), set()
    for c in CASES:
        _, m, kdim, ncols, bits, k, _, _ = c[0]
        for dtype in DTYPES:
            dxs.add(pref.regime_of(c, ops.cbpk_dx_h16_plan(_tdt(dtype), m, kdim, ncols, bits, k, cus), dtype))
            dcs.add(pref.regime_of(c, ops.cbpk_dc_h16_plan(_tdt(dtype), m, kdim, ncols, bits, k, cus), dtype))
    assert pref.required_regimes("dx") <= dxs and pref.required_regimes("dc") <= dcs


# ------------------------------------------------------------------ 1. the lane maps
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits", [2, 4])
def test_identity_g_returns_w_transposed_and_diagonal_x_every_row_of_dw(env, dtype, bits):
    """g = I (m = ncols = 96 > 16: the MFMA tiles) gives dx[r, i] = W_h[i, r] only if the decode puts every field at its (row, column);
    a diagonal x makes dW[i, o] = x[i, i] g[i, o], a value of its own row, so dc equals the float64 bins only if the epilogue of
    k_cbpkdc_mfma reads the label of its own (i, o)."""
    _, ops, _ = env
    m = ncols = 96
    kdim, k = 50, 1 << bits
    rng = np.random.RandomState(5 + bits)
    cen = rng.permutation(np.arange(-8, 8))[:k].astype(np.float32)
    lab = rng.randint(0, k, size=(kdim, ncols))
    codes = _codes(env, lab, bits, k)
    for half_out in (False, True):
        dx = _raw_dx(env, _half(np.eye(m), dtype), dtype, codes, _cuda(cen), half_out)
        assert np.array_equal(dx.float().cpu().numpy(), cen[lab].T), half_out
    kdim, ncols, m = 20, 50, 20
    lab = rng.randint(0, k, size=(kdim, ncols))
    x = np.diag(rng.randint(1, 4, size=kdim)).astype(np.float32)
    g = rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
    dc = _raw_dc(env, _half(x, dtype), _half(g, dtype), dtype, _codes(env, lab, bits, k), True)
    assert np.array_equal(dc.cpu().numpy(), ref.dc64(x, g, lab, k))


# ------------------------------------------------------------------ 2. every case: the references bit for bit, the float64 formulas
@pytest.mark.parametrize("data", ["exact", "float"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", FULL, ids=pref.case_id)
def test_cases_equal_their_references_bit_for_bit(env, case, dtype, data):
    _, ops, cus = env
    (_, m, kdim, ncols, bits, k, _, _), _ = case
    x, g, cen, lab, codes, xt, gt, ct, dense = _case_setup(env, case, dtype, data)
    assert torch.equal(codes.to_dense().reshape(-1), dense)
    tdt = _tdt(dtype)
    cen_h = round_to(cen, dtype)
    w_h = ref.decoded(lab, cen_h)                                             # a label >= K reads 0
    dxp, dcp = ops.cbpk_dx_h16_plan(tdt, m, kdim, ncols, bits, k, cus), ops.cbpk_dc_h16_plan(tdt, m, kdim, ncols, bits, k, cus)
    assert dxp["path"] == dcp["path"] == (h16_ref.PATH_MFMA if m > 16 else h16_ref.PATH_STREAM)
    # dc: the byte form's call on the unpacked labels, both outputs, at every m; the same call gives the same bits
    S, flag = ops.cbgrad_shift(m, np.abs(x).max(), np.abs(g).max(), dcp["terms_log2"])
    for f64 in (True, False):
        dc = _raw_dc(env, xt, gt, dtype, codes, f64)
        want = ops.codebook_centroid_grad(xt, gt, dense, k, kdim, ncols, dtype=torch.float64 if f64 else torch.float32)
        assert _same(dc, want), (f64, (dc.double() - want.double()).abs().max().item())
        assert _same(dc, _raw_dc(env, xt, gt, dtype, codes, f64))
        assert _same(dc, ops.packed_codebook_centroid_grad(xt, gt, codes, dtype=dc.dtype))
        dc64 = ref.dc64(x, g, lab, k)                                         # a label >= K falls into no bin
        if data == "exact":
            assert np.array_equal(dc.cpu().numpy(), dc64.astype(dc.cpu().numpy().dtype))
        elif flag == ops.CBGRAD_OK:
            err, bound = np.abs(dc.double().cpu().numpy() - dc64), href.dc_bound(x, g, lab, k, S, dcp["splits"], not f64)
            WORST["dc"] = max(WORST["dc"], float((err / np.maximum(bound, 1e-300)).max()))
            assert (err <= bound).all()
        if m <= 16:   # also the float32 packed call on the widened inputs
            assert _same(dc, ops.packed_codebook_centroid_grad(xt.float(), gt.float(), codes, dtype=dc.dtype))
    # dx
    dx32, dxh = _raw_dx(env, gt, dtype, codes, ct, False), _raw_dx(env, gt, dtype, codes, ct, True)
    if m > 16:
        assert _same(dx32, ops.codebook_matmul_dx(gt, dense, ct, kdim, ncols, out_dtype=torch.float32))
        assert _same(dxh, ops.codebook_matmul_dx(gt, dense, ct, kdim, ncols))
    else:
        assert _same(dx32, ops.packed_codebook_matmul_dx(gt.float(), codes, ct.to(tdt).float()))
    assert _same(dxh, dx32.to(tdt))                                           # the half output is one rounding of the float32 value
    assert _same(dx32, _raw_dx(env, gt, dtype, codes, ct, False)) and _same(dxh, _raw_dx(env, gt, dtype, codes, ct, True))
    assert _same(dx32, ops.packed_codebook_matmul_dx(gt, codes, ct, out_dtype=torch.float32)) and _same(dxh, ops.packed_codebook_matmul_dx(gt, codes, ct))
    dx64 = g.astype(np.float64) @ w_h.T
    if data == "exact":
        assert np.array_equal(dx32.cpu().numpy(), dx64.astype(np.float32))
        assert np.array_equal(dxh.float().cpu().numpy(), round_to(dx64, dtype))
    else:
        err, bound = np.abs(dx32.double().cpu().numpy() - dx64), href.dx_bound(g, w_h, dxp["splits"])
        WORST["dx"] = max(WORST["dx"], float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in CASES if c not in FULL], ids=pref.case_id)
def test_empty_shapes(env, case, dtype):
    """m = 0 or kdim = 0: dx is empty; ncols = 0: dx = 0; any empty dimension: dc = 0"""
    _, ops, _ = env
    (_, m, kdim, ncols, bits, k, _, _), _ = case
    codes = ops.pack_codes(torch.zeros(kdim * ncols, dtype=torch.uint8, device="cuda"), kdim, ncols, k, bits)
    tdt = _tdt(dtype)
    x, g = torch.ones(m, kdim, dtype=tdt, device="cuda"), torch.ones(m, ncols, dtype=tdt, device="cuda")
    dx = ops.packed_codebook_matmul_dx(g, codes, torch.ones(k, device="cuda"))
    assert dx.shape == (m, kdim) and dx.dtype == tdt and not bool(dx.any())
    for out in (torch.float64, torch.float32):
        dc = ops.packed_codebook_centroid_grad(x, g, codes, dtype=out)
        assert dc.shape == (k,) and dc.dtype == out and not bool(dc.any())


# ------------------------------------------------------------------ 3. the padding trap; m = 16 against m = 17; non-finite inputs
@pytest.mark.parametrize("bits,ncols", [(4, 33), (2, 70)])
@pytest.mark.parametrize("m", [17, 5])
def test_a_centre_zero_that_rounds_to_inf_stays_out_of_the_padding(env, m, bits, ncols):
    """fp16, centers[0] = 1e5 (Inf as fp16), no real weight carries label 0: only the padding fields of a row do.  dx is finite and
    the byte form's; had a padding field been looked up, Inf would have met the zero of the g image (NaN)."""
    _, ops, _ = env
    kdim, k = 40, 1 << bits
    rng = np.random.RandomState(m + bits)
    lab = rng.randint(1, k, size=(kdim, ncols))
    assert (ncols * bits) % 128 != 0 and not (lab == 0).any()
    cen = (rng.randint(-8, 9, size=k) / 4.0).astype(np.float32)
    cen[0] = 1e5
    assert np.isinf(round_to(cen, "fp16")[0])
    g = rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
    codes, gt, ct, dense = _codes(env, lab, bits, k), _half(g, "fp16"), _cuda(cen), _dev_labels(lab)
    for half_out in (False, True):
        dx = _raw_dx(env, gt, "fp16", codes, ct, half_out)
        assert bool(torch.isfinite(dx).all())
        assert _same(dx, ops.codebook_matmul_dx(gt, dense, ct, kdim, ncols, out_dtype=None if half_out else torch.float32))
        assert np.array_equal(dx.float().cpu().numpy(), ref.dx64(g, lab, round_to(cen, "fp16")).astype(np.float32))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bits,k", [(4, 11), (2, 3)])
def test_m16_and_m17_agree_on_exact_data(env, dtype, bits, k):
    """the two sides of the stream / MFMA threshold on the same rows: exact data, so the same values"""
    _, ops, _ = env
    case = (("m17", 17, 129, 200, bits, k, 0, True), False)
    x, g, cen, lab, codes, xt, gt, ct, dense = _case_setup(env, case, dtype, "exact")
    a = ops.packed_codebook_matmul_dx(gt[:16].contiguous(), codes, ct, out_dtype=torch.float32)
    b = ops.packed_codebook_matmul_dx(gt, codes, ct, out_dtype=torch.float32)
    assert torch.equal(a, b[:16])
    d16 = ops.packed_codebook_centroid_grad(xt[:16].contiguous(), gt[:16].contiguous(), codes)
    x17 = xt.clone()
    x17[16] = 0
    assert torch.equal(d16, ops.packed_codebook_centroid_grad(x17, gt, codes))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [7, 40])
def test_nonfinite_inputs(env, dtype, m):
    """an Inf or a NaN in g: dx is the byte form's above 16 rows and the float32 packed call's below, NaN for NaN; dc is all NaN for a
    non-finite x or g"""
    _, ops, _ = env
    kdim, ncols, bits, k = 129, 200, 4, 13
    rng = np.random.RandomState(m)
    lab = rng.randint(0, 16, size=(kdim, ncols))
    cen = (rng.randint(-8, 9, size=k) / 4.0).astype(np.float32)
    codes, ct, dense = _codes(env, lab, bits, k), _cuda(cen), _dev_labels(lab)
    g = rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
    x = rng.randint(-3, 4, size=(m, kdim)).astype(np.float32)
    g[m // 2, 77], g[0, 150] = np.inf, np.nan
    gt, xt = _half(g, dtype), _half(x, dtype)
    for half_out in (False, True):
        dx = _raw_dx(env, gt, dtype, codes, ct, half_out)
        if m > 16:
            assert _same_or_both_nan(dx, ops.codebook_matmul_dx(gt, dense, ct, kdim, ncols, out_dtype=None if half_out else torch.float32))
        else:
            want = ops.packed_codebook_matmul_dx(gt.float(), codes, ct.to(_tdt(dtype)).float())
            assert _same_or_both_nan(dx, want if not half_out else want.to(_tdt(dtype)))
        assert bool(torch.isnan(dx[0]).all()) and not bool(torch.isfinite(dx[m // 2]).any())
    for out in (torch.float64, torch.float32):
        assert bool(torch.isnan(_raw_dc(env, xt, gt, dtype, codes, out == torch.float64)).all())          # the all-NaN rule: g
        x2 = x.copy()
        x2[1, 3] = -np.inf
        g2 = rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
        assert bool(torch.isnan(ops.packed_codebook_centroid_grad(_half(x2, dtype), _half(g2, dtype), codes, dtype=out)).all())   # x


# ------------------------------------------------------------------ 4. the ranges of the two types
@pytest.mark.parametrize("m", [5, 40])
def test_bf16_dc_across_the_exponent_range_and_both_sides_of_p127(env, m):
    """products near 2^-160 (the scaling of section 12 keeps them), and m max|x| max|g| on both sides of 2^127 (above: all NaN):
    the byte form's call bit for bit"""
    _, ops, _ = env
    kdim, ncols, bits, k = 33, 65, 4, 11
    rng = np.random.RandomState(m)
    lab = rng.randint(0, 16, size=(kdim, ncols))
    codes, dense = _codes(env, lab, bits, k), _dev_labels(lab)
    base_x, base_g = rng.randint(-3, 4, size=(m, kdim)).astype(np.float64), rng.randint(-3, 4, size=(m, ncols)).astype(np.float64)
    for ex, eg, nan in ((-80, -80, False), (-120, 10, False), (50, 50, False), (64, 62 - int(np.ceil(np.log2(m * 9))), False), (64, 63, True)):
        xt, gt = _half(base_x * 2.0 ** ex, "bf16"), _half(base_g * 2.0 ** eg, "bf16")
        for out in (torch.float64, torch.float32):
            dc = ops.packed_codebook_centroid_grad(xt, gt, codes, dtype=out)
            assert _same_or_both_nan(dc, ops.codebook_centroid_grad(xt, gt, dense, k, kdim, ncols, dtype=out))
            assert bool(torch.isnan(dc).all()) == nan
            if not nan and out == torch.float64:
                assert np.array_equal(dc.cpu().numpy(), ref.dc64(base_x, base_g, lab, k) * 2.0 ** (ex + eg))


@pytest.mark.parametrize("m", [5, 40])
def test_fp16_extremes(env, m):
    """65504 next to subnormals in x and g: the byte form's call bit for bit, finite"""
    _, ops, _ = env
    kdim, ncols, bits, k = 33, 65, 2, 4
    rng = np.random.RandomState(m)
    lab = rng.randint(0, k, size=(kdim, ncols))
    codes, dense = _codes(env, lab, bits, k), _dev_labels(lab)
    x = rng.choice([65504.0, -65504.0, 2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -14, 1.0, 0.0], size=(m, kdim))
    g = rng.choice([65504.0, 2.0 ** -24, -2.0 ** -20, 1.0, 0.0], size=(m, ncols))
    xt, gt = _half(x, "fp16"), _half(g, "fp16")
    for out in (torch.float64, torch.float32):
        dc = ops.packed_codebook_centroid_grad(xt, gt, codes, dtype=out)
        assert _same(dc, ops.codebook_centroid_grad(xt, gt, dense, k, kdim, ncols, dtype=out)) and bool(torch.isfinite(dc).all())


# ------------------------------------------------------------------ 5. ops.packed_codebook_linear: no host read, dtypes, errors
def _exact_layer(m, kdim=90, ncols=150, k=13, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.randint(-3, 4, size=(m, kdim)).astype(np.float32)
    c = (rng.randint(-8, 9, size=k) / 4.0).astype(np.float32)
    lab = rng.randint(0, k, size=(kdim, ncols))
    b = rng.randint(-4, 5, size=ncols).astype(np.float32)
    return x, c, lab, b


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_forward_plus_backward_makes_no_host_read(env, dtype):
    _, ops, _ = env
    x, c, lab, b = _exact_layer(m=40)
    codes = ops.pack_codes(_dev_labels(lab), 90, 150, 13)
    ct, bt = _cuda(c).requires_grad_(True), _cuda(b).requires_grad_(True)
    xt, x5 = _half(x, dtype).requires_grad_(True), _half(x[:5], dtype).requires_grad_(True)
    gy, gy5 = _half(np.ones((40, 150)), dtype), _half(np.ones((5, 150)), dtype)
    ops.packed_codebook_linear(xt, codes, ct, bias=bt, relu=True).backward(gy)       # (warm: allocations, the library load)
    ops.packed_codebook_linear(x5, codes, ct, bias=bt, relu=True).backward(gy5)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for relu in (False, True):
            y = ops.packed_codebook_linear(xt, codes, ct, bias=bt, relu=relu)
            y.backward(gy)
            ops.packed_codebook_linear(x5, codes, ct, bias=bt, relu=relu).backward(gy5)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert y.dtype == _tdt(dtype) and xt.grad.dtype == _tdt(dtype) and ct.grad.dtype == torch.float32 and bt.grad.dtype == torch.float32


def test_dtype_errors(env):
    _, ops, _ = env
    x, c, lab, b = _exact_layer(m=3)
    codes = ops.pack_codes(_dev_labels(lab), 90, 150, 13)
    ct, bt = _cuda(c), _cuda(b)
    g, xh = _half(np.ones((3, 150)), "bf16"), _half(x, "bf16")
    with pytest.raises(TypeError):
        ops.packed_codebook_matmul_dx(g, codes, ct.bfloat16())
    with pytest.raises(TypeError):
        ops.packed_codebook_matmul_dx(g, codes, ct, out_dtype=torch.float16)
    with pytest.raises(TypeError):
        ops.packed_codebook_matmul_dx(g.float(), codes, ct, out_dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="one dtype"):
        ops.packed_codebook_centroid_grad(xh, g.half(), codes)
    with pytest.raises(TypeError, match="one dtype"):
        ops.packed_codebook_centroid_grad(xh.float(), g, codes)
    with pytest.raises(TypeError):
        ops.packed_codebook_linear(xh, codes, ct.bfloat16())
    with pytest.raises(TypeError):
        ops.packed_codebook_linear(xh, codes, ct, bias=bt.bfloat16())
    assert ops.packed_codebook_matmul_dx(g, codes, ct).dtype == torch.bfloat16
    assert ops.packed_codebook_matmul_dx(g.float(), codes, ct, out_dtype=torch.float32).dtype == torch.float32


# ------------------------------------------------------------------ 6. the layers
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", [None, torch.relu])
def test_packed_and_byte_trainable_dense_agree_bit_for_bit(env, dtype, act):
    """m > 16: a TrainablePackedCompressedDense(half_inputs=True) and a TrainableCompressedDense(half_inputs=True) on to_dense() give
    the same output, x.grad, centers.grad and bias.grad, float data, with a fused ReLU too"""
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    rng = np.random.RandomState(3)
    kdim, ncols, k, m = 129, 200, 13, 40
    lab = rng.randint(0, k, size=(kdim, ncols))
    labels, ct, bt = _dev_labels(lab), _cuda((rng.randn(k) * 0.1).astype(np.float32)), _cuda(rng.randn(ncols).astype(np.float32))
    codes = ops.pack_codes(labels, kdim, ncols, k)
    packed = compressed.TrainablePackedCompressedDense(codes, labels, ct, bt, None, act, half_inputs=True)
    byte = compressed.TrainableCompressedDense(kdim, ncols, codes.to_dense(), ct, bt, None, act, half_inputs=True)
    assert packed.half_inputs and torch.equal(packed.kernel_sq_sum(), byte.kernel_sq_sum())
    x = rng.randn(m, kdim)
    gy = _half(rng.randn(m, ncols) * 0.01, dtype)
    outs = []
    for layer in (packed, byte):
        layer.bias.requires_grad_(True)
        xt = _half(x, dtype).requires_grad_(True)
        y = layer(xt)
        y.backward(gy)
        outs.append((y.detach(), xt.grad, layer.centers.grad, layer.bias.grad))
    assert outs[0][0].dtype == _tdt(dtype) and outs[0][1].dtype == _tdt(dtype) and outs[0][2].dtype == torch.float32
    for a, b in zip(*outs):
        assert _same(a, b)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ks,cin,cout,pad,hw", [(5, 1, 6, 0, 12), (3, 4, 8, 1, 7)])
def test_trainable_packed_conv_with_half_inputs(env, dtype, ks, cin, cout, pad, hw):
    """exact data: the layer's output and centre gradient are the float64 formulas on the patches"""
    from neural_network_compression_amd import compressed

    rng = np.random.RandomState(ks)
    k, kdim = 9, ks * ks * cin
    lab = rng.randint(0, k, size=kdim * cout).astype(np.uint8)
    c = (rng.randint(-4, 5, size=k) / 4.0).astype(np.float32)
    lab_t = _cuda(lab)
    lab_u = compressed._unfold_labels(ks, cin, cout, lab_t)
    layer = compressed.TrainablePackedCompressedConv2D.from_codes(ks, cin, cout, pad, lab_t, _cuda(c), half_inputs=True)
    x = rng.randint(-2, 3, size=(3, hw, hw, cin)).astype(np.float32)
    xt = _half(x, dtype).requires_grad_(True)
    y = layer(xt)
    ho = hw + 2 * pad - ks + 1
    assert y.dtype == _tdt(dtype) and y.shape == (3, ho, ho, cout)
    patches = compressed.conv_patches(xt.detach(), ks, pad).contiguous().reshape(-1, kdim)
    lab2d = lab_u.cpu().numpy().reshape(kdim, cout)
    p64 = patches.double().cpu().numpy()
    assert np.array_equal(y.detach().float().cpu().numpy().reshape(-1, cout), round_to(p64 @ ref.decoded(lab2d, c), dtype))
    gy = rng.randint(-2, 3, size=tuple(y.shape)).astype(np.float32)
    y.backward(_half(gy, dtype))
    assert np.array_equal(layer.centers.grad.cpu().numpy(), ref.dc64(p64, gy.reshape(-1, cout), lab2d, k).astype(np.float32))
    assert xt.grad.dtype == _tdt(dtype) and xt.grad.shape == xt.shape
    byte = compressed.TrainableCompressedConv2D(ks, cin, cout, pad, lab_u, _cuda(c), None, None, None, half_inputs=True)
    xb = _half(x, dtype).requires_grad_(True)
    byte(xb).backward(_half(gy, dtype))
    assert _same(xb.grad, xt.grad)
    with pytest.raises(TypeError, match="float32 activations"):
        compressed.TrainablePackedCompressedConv2D.from_codes(ks, cin, cout, pad, lab_t, _cuda(c))(xt.detach())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [5, 40])
def test_two_layer_chain_with_exact_data_is_float64_autograd(env, m, dtype):
    """20 -> 24 -> 10 with x in {-1, 0, 1} (4 non-zeros a row), first centres multiples of 1/2 in [-1, 1], second in {-1, 0, 1},
    upstream gradient in {-1, 0, 1}: every intermediate is exact in the dtype (asserted in float64), so all centre gradients equal
    float64 autograd on the decoded weights bit for bit"""
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    rng = np.random.RandomState(m)
    x = np.zeros((m, 20))
    for r in range(m):
        x[r, rng.choice(20, 4, replace=False)] = rng.choice([-1.0, 1.0], 4)
    c1, c2 = np.array([-1, -0.5, 0, 0.5, 1], dtype=np.float32), np.array([-1, 0, 1], dtype=np.float32)
    lab1, lab2 = rng.choice(5, size=(20, 24), p=[0.1, 0.1, 0.6, 0.1, 0.1]), rng.choice(3, size=(24, 10), p=[0.2, 0.6, 0.2])
    gy = rng.randint(-1, 2, size=(m, 10)).astype(np.float64)
    w1, w2 = torch.from_numpy(ref.decoded(lab1, c1)).requires_grad_(True), torch.from_numpy(ref.decoded(lab2, c2)).requires_grad_(True)
    h = torch.from_numpy(x) @ w1
    h.retain_grad()
    y = h @ w2
    y.backward(torch.from_numpy(gy))
    for t in (h.detach(), y.detach(), h.grad):                 # the precondition: exact in the dtype
        assert np.array_equal(round_to(t.numpy(), dtype), t.numpy())
    layers = []
    for kd, nc, lab, c in ((20, 24, lab1, c1), (24, 10, lab2, c2)):
        layers.append(compressed.TrainablePackedCompressedDense.from_codes(kd, nc, _dev_labels(lab), _cuda(c), half_inputs=True))
    assert (layers[0].bits, layers[1].bits) == (4, 2)
    out = layers[1](layers[0](_half(x, dtype)))
    assert np.array_equal(out.detach().float().cpu().numpy(), y.detach().numpy())
    out.backward(_half(gy, dtype))
    for layer, w, lab, k in ((layers[0], w1, lab1, 5), (layers[1], w2, lab2, 3)):
        assert np.array_equal(layer.centers.grad.cpu().numpy(), ref.bin64(w.grad.numpy(), lab, k).astype(np.float32))


def test_without_the_option_half_inputs_raise_and_float32_keeps_its_bits(env):
    """Plain layers still raise TypeError on a half input.  A float32 input through every packed trainable layer, built either way,
    gives the bits of ops.packed_codebook_matmul_dx / packed_codebook_centroid_grad on float32."""
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    rng = np.random.RandomState(11)
    kdim, ncols, k = 129, 100, 13
    lab = rng.randint(0, k, size=(kdim, ncols))
    labels, ct = _dev_labels(lab), _cuda((rng.randn(k) * 0.1).astype(np.float32))
    codes = ops.pack_codes(labels, kdim, ncols, k)
    built = [compressed.TrainablePackedCompressedDense.from_codes(kdim, ncols, labels, ct),
             compressed.TrainablePackedCompressedDense(codes, labels, ct),
             compressed.TrainablePackedCompressedDense(codes, labels, ct, half_inputs=True)]
    assert [b.half_inputs for b in built] == [False, False, True]
    for m in (7, 40):
        x, g = torch.randn(m, kdim, device="cuda"), torch.randn(m, ncols, device="cuda") * 0.01
        dx, dc = ops.packed_codebook_matmul_dx(g, codes, ct), ops.packed_codebook_centroid_grad(x, g, codes, dtype=torch.float32)
        for layer in built:
            layer.centers.grad = None
            xt = x.clone().requires_grad_(True)
            layer(xt).backward(g)
            assert _same(xt.grad, dx) and _same(layer.centers.grad, dc)
    for tdt in (torch.bfloat16, torch.float16):
        for layer in built[:2]:
            with pytest.raises(TypeError, match="float32 activations"):
                layer(torch.zeros(3, kdim, dtype=tdt, device="cuda"))
        assert built[2](torch.zeros(3, kdim, dtype=tdt, device="cuda")).dtype == tdt


# ------------------------------------------------------------------ 7. the trainer
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


def test_one_batch_of_fine_tune_compressed_packed_in_bf16_is_the_step_from_the_ops_calls(env, quantized):
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    t, tr, data, test = quantized
    models = t.quantized_models_by_layer
    dt, lr = torch.bfloat16, 1e-2
    c0 = _centres(models)
    names = ("dense1", "dense2", "out")
    layers = [getattr(t.neural_network, n) for n in names]
    net = compressed.compress_network_trainable(t.neural_network, models, packed=True, packed_half_inputs=True)
    assert all(isinstance(l, compressed.TrainablePackedCompressedDense) and l.half_inputs for l in net.get_config().values())
    auto = compressed.compress_network_trainable(t.neural_network, models, packed="auto", packed_half_inputs=True)
    plain = compressed.compress_network_trainable(t.neural_network, models, packed="auto")
    assert [type(a) for a in auto.get_config().values()] == [type(p) for p in plain.get_config().values()]      # what "auto" picks does not change
    assert all(l.half_inputs for l in auto.get_config().values())
    both = compressed.compress_network_trainable(t.neural_network, models, sparse="auto", packed="auto", sparse_half_inputs=True, packed_half_inputs=True)
    assert all(l.half_inputs for l in both.get_config().values())
    # the step from the ops calls, on the batch fine_tune_compressed will draw
    torch.manual_seed(5)
    xb, yb = next(tr._batches(t._to_device(data.input_data).float(), t._to_device(data.output_data).float()))
    cs = [torch.from_numpy(c0[(l, 0)]).cuda() for l in layers]
    bcs = [torch.from_numpy(c0[(l, 1)]).cuda() if (l, 1) in c0 else None for l in layers]
    labs = [models[l][0].labels_compact_ for l in layers]
    blabs = [models[l][1].labels_compact_ if (l, 1) in c0 else None for l in layers]
    biases = [ops.gather(bcs[i], blabs[i]) if bcs[i] is not None else layers[i].bias.detach() for i in range(3)]
    shapes = [tuple(l.kernel.shape) for l in layers]
    codes = [ops.pack_codes(labs[i], *shapes[i], cs[i].numel()) for i in range(3)]
    acts = [xb.to(dt)]
    with torch.no_grad():
        for i in range(3):
            acts.append(ops.packed_codebook_matmul(acts[-1], codes[i], cs[i], bias=biases[i], relu=i < 2))
    logits = acts[-1].float().requires_grad_(True)
    torch.nn.functional.binary_cross_entropy_with_logits(logits, yb).backward()
    g = logits.grad.to(dt)
    want = {}
    for i in (2, 1, 0):
        if i < 2:
            g = torch.where(acts[i + 1] > 0, g, torch.zeros((), dtype=dt, device="cuda"))
        dc = ops.packed_codebook_centroid_grad(acts[i], g, codes[i], dtype=torch.float32)
        assert torch.equal(dc, ops.codebook_centroid_grad(acts[i], g, labs[i], cs[i].numel(), *shapes[i], dtype=torch.float32))
        cp = cs[i].clone().requires_grad_(True)
        counts = ops.bincount(labs[i], cs[i].numel())
        (0.01 * ((counts.to(torch.float32) * cp ** 2).sum() / 2)).backward()
        want[(layers[i], 0)] = (cs[i], dc, cp.grad)
        if bcs[i] is not None:
            db = ops.centroid_gradient(g.sum(0, dtype=torch.float32).contiguous(), blabs[i], bcs[i].numel()).to(torch.float32)
            want[(layers[i], 1)] = (bcs[i], db, None)
        if i > 0:
            g = ops.packed_codebook_matmul_dx(g, codes[i], cs[i])

    kw = dict(packed=True, activation_dtype=dt, packed_half_inputs=True)
    torch.manual_seed(5)
    t.fine_tune_compressed(data, test, epochs=1, learning_rate=0.0, **kw)
    assert all(np.array_equal(c, c0[key]) for key, c in _centres(models).items())      # learning_rate = 0: bit-identical
    torch.manual_seed(5)
    t.fine_tune_compressed(data, test, epochs=1, learning_rate=lr, **kw)
    got = _centres(models)                                                               # the write-back: the tuned centres reached the models
    try:
        for key, (c, grad, l2) in want.items():
            steps = [c - lr * (grad + l2), c - lr * (l2 + grad)] if l2 is not None else [c - lr * grad]
            assert any(np.array_equal(got[key], s.cpu().numpy()) for s in steps), key
            assert not np.array_equal(got[key], c0[key])
        for layer in layers:                                                             # and the float layers are re-decoded
            assert torch.equal(layer.kernel.detach().reshape(-1), ops.gather(torch.from_numpy(got[(layer, 0)]).cuda(), models[layer][0].labels_compact_))
    finally:
        for (layer, ti), c in c0.items():                                                # leave the shared fixture as it was
            models[layer][ti].cluster_centers_ = c.reshape(-1, 1).copy()


def test_fine_tune_compressed_packed_half_errors(env, quantized):
    t, tr, data, test = quantized
    for kw in (dict(packed=True), dict(packed="auto")):                                  # pinned: without the new keyword
        with pytest.raises(ValueError, match="the packed forms do not train"):
            t.fine_tune_compressed(data, test, epochs=1, activation_dtype=torch.bfloat16, **kw)
    with pytest.raises(ValueError, match="packed_half_inputs"):
        t.fine_tune_compressed(data, test, epochs=1, packed=True, packed_half_inputs=True)
    with pytest.raises(ValueError, match="packed_half_inputs"):
        t.fine_tune_compressed(data, test, epochs=1, activation_dtype=torch.bfloat16, packed_half_inputs=True)
    with pytest.raises(ValueError, match="sparse_half_inputs"):
        t.fine_tune_compressed(data, test, epochs=1, activation_dtype=torch.bfloat16, sparse="auto", packed="auto", packed_half_inputs=True)
    with pytest.raises(ValueError):
        t.compressed_network(trainable=True, packed=True, packed_half_inputs=True)
    models = t.quantized_models_by_layer
    kept = models[t.neural_network.dense2]
    models[t.neural_network.dense2] = [None, None]              # dense2 passed through unquantized
    try:
        with pytest.raises(ValueError, match="dense2"):
            t.fine_tune_compressed(data, test, epochs=1, packed=True, activation_dtype=torch.float16, packed_half_inputs=True)
    finally:
        models[t.neural_network.dense2] = kept


def test_print_the_largest_error_over_bound(env):
    """the float-data cases above, against section 22's derived bounds (the second, looser check): the largest err / bound"""
    print(f"\npacked h16 backward, float data: max err / bound  dx {WORST['dx']:.3g}  dc {WORST['dc']:.3g}")
    assert WORST["dx"] <= 1.0 and WORST["dc"] <= 1.0
