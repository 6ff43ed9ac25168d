"""The backward pass of the bitmap-sparse codebook layer on bf16 / fp16 activations (nnc_cbsp_dx_h16 / nnc_cbsp_dc_h16,
csrc/nnc_cbspgrad_h16.hip), through the raw C ABI with buffers the test owns, through ops.sparse_codebook_*
and ops.sparse_codebook_linear, through the trainable sparse layers built with half_inputs=True and through
Trainer.fine_tune_compressed(sparse=..., activation_dtype=..., sparse_half_inputs=True) (run with -m gpu).

What it is held to needs no tolerance but the float-data bound.  dc equals ops.codebook_centroid_grad on the unpacked labels and the
same half inputs bit for bit at every m.  Above 16 rows dx equals ops.codebook_matmul_dx on the unpacked labels bit for bit, non-finite
g included; up to 16 rows the float32 dx is ops.sparse_codebook_matmul_dx on the widened g and the rounded centres bit for bit and a
half dx is that value rounded once.  On exact data (integer x and g in [-3, 3], centres multiples of 1/4 in [-2, 2]: every partial
sum is exact in float32 in any order) all of them equal the float64 formulas.  Every raw call writes into sentinel-framed outputs and
workspace, reads x and g directly in front of NaN bit patterns and the symbols at the very end of their tensor, and is repeated for
the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_compression_amd import synth  # noqa: E402
from tests.helpers import cbgrad_ref as ref  # noqa: E402
from tests.helpers import h16_grad_ref as href  # noqa: E402
from tests.helpers import h16_ref  # noqa: E402
from tests.helpers import sparse_h16_grad_ref as sref  # noqa: E402
from tests.helpers.h16_ref import DTYPES, round_to  # noqa: E402
from tests.helpers.sparse_h16_grad_ref import CASES  # noqa: E402

SENT16 = 0x7FA5              # as bf16 and as fp16 a NaN whose payload neither the inputs nor the kernels' own NaNs carry
SENT32 = 0x7FA57FA5
SENT64 = 0x7FA57FA57FA57FA5
WS_PAD = 64


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


def _dev_labels(lab, lb):
    host = np.ascontiguousarray(lab, dtype=np.uint8 if lb == 1 else np.uint16).ravel()
    return torch.from_numpy(host if lb == 1 else host.view(np.int16)).cuda()


def _codes(env, lab, lb, k, z):
    """The packed form of lab (kdim, ncols), moved so that its last symbol is the last byte of its tensor (256 bytes of 0xFF in front
    keep the alignment).  z None: the packer's own choice."""
    _, ops, _ = env
    kdim, ncols = lab.shape
    codes = ops.pack_sparse_codes(_dev_labels(lab, lb), kdim, ncols, k, zero_symbol=z)
    assert codes.nnz == int((lab != codes.zero_symbol).sum())
    big = torch.full((256 + codes.nbytes(),), 255, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 256 == 0
    big[256:] = codes.buf
    return ops.SparseCodes(big[256:], kdim, ncols, k, codes.zero_symbol, lb, codes.nnz)


def _framed(units, pad, sent, tdtype):
    buf = torch.full((units + 2 * pad,), sent, dtype=tdtype, device="cuda")
    return buf, buf[pad: pad + units]


def _raw_dx(env, g, dtype, codes, centers, half_out):
    """nnc_cbsp_dx_h16 into sentinel-framed dx and workspace (exactly the queried size); checks the frames; returns dx (m, kdim)."""
    L, ops, _ = env
    m, kdim, ncols, lb = g.shape[0], codes.kdim, codes.ncols, codes.label_bytes
    ws_bytes = int(L.nnc_cbsp_dx_h16_workspace_bytes(m, kdim, ncols, lb))
    assert ws_bytes % 4 == 0
    units, pad = (m * kdim, 37) if half_out else (2 * m * kdim, 38)
    obuf, out = _framed(units, pad, SENT16, torch.int16)
    wbuf, ws = _framed(ws_bytes // 4, WS_PAD, SENT32, torch.int32)
    dt = h16_ref.DT_CODE[dtype]
    ops.nat.check(L.nnc_cbsp_dx_h16(g.data_ptr(), dt, m, kdim, codes.buf.data_ptr(), codes.nbytes(), lb, ncols, codes.zero_symbol, codes.nnz,
                                    centers.data_ptr(), centers.numel(), out.data_ptr(), dt if half_out else 0, ws.data_ptr() if ws_bytes else None,
                                    ws_bytes, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((obuf[:pad] == SENT16).all()) and bool((obuf[pad + units:] == SENT16).all()), "a store outside dx"
    assert bool((wbuf[:WS_PAD] == SENT32).all()) and bool((wbuf[WS_PAD + ws_bytes // 4:] == SENT32).all()), "a store outside the workspace"
    if half_out:
        assert not bool((out == SENT16).any()), "an output left unwritten"
        return out.clone().view(_tdt(dtype)).view(m, kdim)
    assert not bool((out.view(torch.int32) == SENT32).any()), "an output left unwritten"
    return out.clone().view(torch.float32).view(m, kdim)


def _raw_dc(env, x, g, dtype, codes, f64):
    """nnc_cbsp_dc_h16 into sentinel-framed dc and workspace; checks the frames; returns dc [k]."""
    L, ops, _ = env
    m, kdim, ncols, lb, k = x.shape[0], codes.kdim, codes.ncols, codes.label_bytes, codes.k
    ws_bytes = int(L.nnc_cbsp_dc_h16_workspace_bytes(m, kdim, ncols, lb, k))
    assert ws_bytes == 64 + 8 * k
    obuf, out = _framed(k if f64 else k, 8, SENT64 if f64 else SENT32, torch.int64 if f64 else torch.int32)
    wbuf, ws = _framed(ws_bytes // 8, WS_PAD, SENT64, torch.int64)
    ops.nat.check(L.nnc_cbsp_dc_h16(x.data_ptr(), g.data_ptr(), h16_ref.DT_CODE[dtype], m, kdim, codes.buf.data_ptr(), codes.nbytes(), lb, ncols,
                                    codes.zero_symbol, codes.nnz, k, out.data_ptr(), 1 if f64 else 0, ws.data_ptr(), ws_bytes,
                                    torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    sent = SENT64 if f64 else SENT32
    assert bool((obuf[:8] == sent).all()) and bool((obuf[8 + k:] == sent).all()), "a store outside dc"
    assert bool((wbuf[:WS_PAD] == SENT64).all()) and bool((wbuf[WS_PAD + ws_bytes // 8:] == SENT64).all()), "a store outside the workspace"
    assert not bool((out == sent).any()), "a bin left unwritten"
    return out.clone().view(torch.float64 if f64 else torch.float32)


def _case_setup(env, c, dtype, data):
    """(x, g, centres, labels (kdim, ncols), codes, x_t, g_t, c_t, dense labels tensor) of a case: exact or float data, rounded to dtype"""
    lab, z = sref.case_labels(c)
    m, kdim, ncols, k, lb = c["m"], c["kdim"], c["ncols"], c["k"], c["lb"]
    rng = np.random.RandomState(17 + m + 3 * kdim + 5 * ncols)
    if data == "exact":
        x = rng.randint(-3, 4, size=(m, kdim)).astype(np.float32)
        g = rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
        cen = (rng.randint(-8, 9, size=k) / 4.0).astype(np.float32)
    else:
        x = round_to(rng.randn(m, kdim), dtype)
        g = round_to(rng.randn(m, ncols) * 0.01, dtype)
        cen = (np.sort(rng.randn(k)) * 0.08).astype(np.float32)
    codes = _codes(env, lab, lb, k, z)
    return x, g, cen, lab, codes, _half(x, dtype, c["view"]), _half(g, dtype, c["view"]), _cuda(cen), _dev_labels(lab, lb)


def test_every_regime_is_covered_at_this_cu_count(env):
    _, ops, cus = env
    dxs, dcs = set(), set()
    for c in CASES:
        for dtype in DTYPES:
            dxs.add(sref.regime_of(c, ops.cbsp_dx_h16_plan(_tdt(dtype), c["m"], c["kdim"], c["ncols"], c["lb"], c["k"], cus), dtype))
            dcs.add(sref.regime_of(c, ops.cbsp_dc_h16_plan(_tdt(dtype), c["m"], c["kdim"], c["ncols"], c["lb"], c["k"], cus), dtype))
    assert sref.required_regimes("dx") <= dxs and sref.required_regimes("dc") <= dcs


# ------------------------------------------------------------------ 1. the lane maps
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lb", [1, 2])
def test_identity_g_returns_w_transposed_and_diagonal_x_every_dw(env, dtype, lb):
    """g = I (m = ncols = 96 > 16: the MFMA tiles) gives dx[r, i] = W_h[i, r] only if the decode puts every symbol at its (row, column);
    a diagonal x gives every dW its own bin only if the epilogue of k_cbspdc_mfma reads the label of its own (i, o)."""
    _, ops, _ = env
    m = ncols = 96
    kdim, k, z = 50, 256, 5
    rng = np.random.RandomState(5 + lb)
    cen = rng.permutation(np.arange(-128, 128)).astype(np.float32)        # exact in bf16 and fp16; cen[z] != 0
    from tests.helpers.sparse_ref import labels_at_density
    lab = labels_at_density(rng, kdim, ncols, k, 0.3, z)
    w = cen[lab]
    codes = _codes(env, lab, lb, k, z)
    for half_out in (False, True):
        dx = _raw_dx(env, _half(np.eye(m), dtype), dtype, codes, _cuda(cen), half_out)
        assert np.array_equal(dx.float().cpu().numpy(), w.T), half_out
    kdim, ncols, m, k = 20, 50, 20, 1000
    lab = np.arange(k).reshape(kdim, ncols)
    lab[rng.rand(kdim, ncols) < 0.6] = 999                                 # most positions skipped: they share bin 999
    x = np.diag(np.arange(1, kdim + 1)).astype(np.float32)
    g = rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
    want = ref.bin64(np.arange(1, kdim + 1)[:, None] * g.astype(np.float64), lab, k)
    codes = _codes(env, lab, 2, k, 999)
    dc = _raw_dc(env, _half(x, dtype), _half(g, dtype), dtype, codes, True)
    assert np.array_equal(dc.cpu().numpy(), want)


# ------------------------------------------------------------------ 2. every case: the references bit for bit, the float64 formulas
def _float_dx_bound(c, g, w_h, cz, splits):
    """Section 22's bound with the decoded W_h, (ncols + splits + 2) 2^-23 sum_o |g| |W_h|.  Up to 16 rows the kernel forms
    c_z sum_o g + sum_stored g (c - c_z) instead: the same count of float32 roundings (one per product-sum step, one per split, the
    rank-1 product and its addition, the difference c - c_z) on terms bounded by |g| (|W_h| + 2 |c_z|), so that magnitude and two
    more roundings bound it."""
    if c["m"] > 16:
        return href.dx_bound(g, w_h, splits)
    mag = np.abs(g.astype(np.float64)) @ (np.abs(w_h) + 2 * abs(cz)).T
    return (c["ncols"] + splits + 4) * href.U32 * mag


@pytest.mark.parametrize("data", ["exact", "float"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c", CASES, ids=sref.case_id)
def test_cases_equal_their_references_bit_for_bit(env, c, dtype, data):
    _, ops, cus = env
    m, kdim, ncols, k, lb = c["m"], c["kdim"], c["ncols"], c["k"], c["lb"]
    x, g, cen, lab, codes, xt, gt, ct, dense = _case_setup(env, c, dtype, data)
    assert torch.equal(codes.to_dense().reshape(-1), dense)
    cen_h = round_to(cen, dtype)
    w_h = ref.decoded(lab, cen_h)
    z = codes.zero_symbol
    cz = float(cen_h[z]) if z < k else 0.0
    # dc: the byte form's call on the unpacked labels, both outputs, at every m; the same call gives the same bits
    dxp, dcp = (ops.cbsp_dx_h16_plan(_tdt(dtype), m, kdim, ncols, lb, k, cus), ops.cbsp_dc_h16_plan(_tdt(dtype), m, kdim, ncols, lb, k, cus))
    S, flag = ops.cbgrad_shift(m, np.abs(x).max(), np.abs(g).max(), dcp["terms_log2"])
    for f64 in (True, False):
        dc = _raw_dc(env, xt, gt, dtype, codes, f64)
        want = ops.codebook_centroid_grad(xt, gt, dense, k, kdim, ncols, dtype=torch.float64 if f64 else torch.float32)
        assert _same(dc, want), (f64, (dc.double() - want.double()).abs().max().item())
        assert _same(dc, _raw_dc(env, xt, gt, dtype, codes, f64))
        assert _same(dc, ops.sparse_codebook_centroid_grad(xt, gt, codes, dtype=dc.dtype))
        dc64 = ref.dc64(x, g, lab, k)
        if data == "exact":
            assert np.array_equal(dc.cpu().numpy(), dc64.astype(dc.cpu().numpy().dtype))
        elif flag == ops.CBGRAD_OK:
            assert (np.abs(dc.double().cpu().numpy() - dc64) <= href.dc_bound(x, g, lab, k, S, dcp["splits"], not f64)).all()
        if m <= 16:   # also the float32 sparse call on the widened inputs
            assert _same(dc, ops.sparse_codebook_centroid_grad(xt.float(), gt.float(), codes, dtype=dc.dtype))
    # dx
    dx32, dxh = _raw_dx(env, gt, dtype, codes, ct, False), _raw_dx(env, gt, dtype, codes, ct, True)
    if m > 16:
        assert _same(dx32, ops.codebook_matmul_dx(gt, dense, ct, kdim, ncols, out_dtype=torch.float32))
        assert _same(dxh, ops.codebook_matmul_dx(gt, dense, ct, kdim, ncols))
    else:
        want = ops.sparse_codebook_matmul_dx(gt.float(), codes, ct.to(_tdt(dtype)).float())
        assert _same(dx32, want)
    assert _same(dxh, dx32.to(_tdt(dtype)))                                  # the half output is one rounding of the float32 value
    assert _same(dx32, _raw_dx(env, gt, dtype, codes, ct, False)) and _same(dxh, _raw_dx(env, gt, dtype, codes, ct, True))
    assert _same(dx32, ops.sparse_codebook_matmul_dx(gt, codes, ct, out_dtype=torch.float32)) and _same(dxh, ops.sparse_codebook_matmul_dx(gt, codes, ct))
    dx64 = g.astype(np.float64) @ w_h.T
    if data == "exact":
        assert np.array_equal(dx32.cpu().numpy(), dx64.astype(np.float32))
        assert np.array_equal(dxh.float().cpu().numpy(), round_to(dx64, dtype))
    else:
        assert (np.abs(dx32.double().cpu().numpy() - dx64) <= _float_dx_bound(c, g, w_h, cz, dxp["splits"])).all()


# ------------------------------------------------------------------ 3. non-finite g; m = 16 against m = 17
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lb,k", [(1, 200), (2, 300)])
def test_nonfinite_g_follows_the_byte_form_above_16_rows_and_stays_out_below(env, dtype, lb, k):
    """m > 16: an Inf in g at a column where row i is skipped gives Inf * 0 = NaN in dx[r, i], as in the byte form (the departure from
    nnc_cbsp_dx_f32), bit for bit with ops.codebook_matmul_dx, NaN for NaN.  m <= 16: with rn(c_z) == 0 a skipped weight forms no
    product, so the Inf reaches only the rows that store that column."""
    _, ops, _ = env
    kdim, ncols, z = 129, 200, 3
    rng = np.random.RandomState(lb)
    from tests.helpers.sparse_ref import labels_at_density
    lab = labels_at_density(rng, kdim, ncols, k, 0.3, z)
    cen = (rng.randint(-8, 9, size=k) / 4.0).astype(np.float32)
    cen[z] = 2.0 ** -140 if dtype == "fp16" else 0.0                       # fp16: rounds to 0; bf16: 0
    cen[cen == 0] = 0.25
    cen[z] = 2.0 ** -140 if dtype == "fp16" else 0.0
    codes, ct, dense = _codes(env, lab, lb, k, z), _cuda(cen), _dev_labels(lab, lb)
    for m in (7, 16, 17, 130):
        g = rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
        g[m // 2, 77] = np.inf
        g[0, 150] = np.nan
        gt = _half(g, dtype)
        for half_out in (False, True):
            dx = _raw_dx(env, gt, dtype, codes, ct, half_out)
            if m > 16:
                assert _same_or_both_nan(dx, ops.codebook_matmul_dx(gt, dense, ct, kdim, ncols, out_dtype=None if half_out else torch.float32))
                stored = torch.from_numpy(lab[:, 77] != z).cuda()          # every row i meets the Inf: Inf * c where stored, Inf * 0 where skipped
                row = dx[m // 2].float()
                assert bool(torch.isinf(row[stored]).all()) and bool(torch.isnan(row[~stored]).all())
            else:
                want = ops.sparse_codebook_matmul_dx(gt.float(), codes, ct.to(_tdt(dtype)).float())
                assert _same_or_both_nan(dx, want if not half_out else want.to(_tdt(dtype)))
                stored = torch.from_numpy(lab[:, 77] != z).cuda()
                row = dx[m // 2].float()
                assert bool(torch.isfinite(row[~stored]).all()) and not bool(torch.isfinite(row[stored]).any())
        dc = ops.sparse_codebook_centroid_grad(gt[:, :kdim].contiguous(), gt, codes)
        assert bool(torch.isnan(dc).all())                                  # the all-NaN rule


@pytest.mark.parametrize("dtype", DTYPES)
def test_m16_and_m17_agree_on_exact_data(env, dtype):
    """the two sides of the stream / MFMA threshold on the same rows: exact data, so the same values"""
    _, ops, _ = env
    c = dict(m=17, kdim=129, ncols=200, lb=1, k=256, density=0.32, z="given", beyond=True, view=False)
    x, g, cen, lab, codes, xt, gt, ct, dense = _case_setup(env, c, dtype, "exact")
    a = ops.sparse_codebook_matmul_dx(gt[:16].contiguous(), codes, ct, out_dtype=torch.float32)
    b = ops.sparse_codebook_matmul_dx(gt, codes, ct, out_dtype=torch.float32)
    assert torch.equal(a, b[:16])
    d16 = ops.sparse_codebook_centroid_grad(xt[:16].contiguous(), gt[:16].contiguous(), codes)
    x17, g17 = xt.clone(), gt.clone()
    x17[16] = 0
    assert torch.equal(d16, ops.sparse_codebook_centroid_grad(x17, g17, codes))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lb", [1, 2])
def test_a_row_whose_count_crosses_2_pow_32(env, dtype, lb):
    """The count of a segment is hi[i] << 32 | lo[segment], plus 2^32 where lo wrapped inside the row (lo < lo[first segment of the
    row]).  A layer of 4 G stored symbols is not a quick test, so the counters of a small form are moved instead: 2^32 - (the count in
    the middle of row r) is added to every count from row r on.  Row r then starts just below 2^32 and wraps between two of its
    segments, the rows behind it start above 2^32.  Every position from row r on now lies past the nnz stored symbols, which reads as
    skipped (as nnc_cbsp_unpack reads it) -- but only if the carry is applied: without it the wrapped segments of row r would read
    the first symbols of the stream.  No symbol load leaves the buffer either way."""
    _, ops, _ = env
    kdim, ncols, k, z, r = 40, 200, 30, 4, 21
    segs = -(-ncols // 64)
    rng = np.random.RandomState(lb)
    from tests.helpers.sparse_ref import labels_at_density
    lab = labels_at_density(rng, kdim, ncols, k, 0.5, z)
    codes = _codes(env, lab, lb, k, z)
    stored = np.zeros((kdim, segs * 64), dtype=np.int64)
    stored[:, :ncols] = lab != z
    per_seg = stored.reshape(kdim, segs, 64).sum(axis=2).ravel()
    counts = np.concatenate([[0], np.cumsum(per_seg)[:-1]]).reshape(kdim, segs)           # the exclusive count of every segment
    assert per_seg.reshape(kdim, segs)[r, :2].sum() > 0 and per_seg.reshape(kdim, segs)[r, 2:].sum() > 0
    moved = counts.copy()
    moved[r:] += 2 ** 32 - int(counts[r, 2])                                              # row r wraps in front of its third segment
    assert moved[r, 0] < 2 ** 32 <= moved[r, 2] and (moved[r, 2] & 0xFFFFFFFF) < (moved[r, 0] & 0xFFFFFFFF)
    G = kdim * segs
    lo = codes.buf[8 * G: 12 * G].view(torch.int32)
    hi = codes.buf[12 * G: 12 * G + 4 * kdim].view(torch.int32)
    assert np.array_equal(lo.cpu().numpy().view(np.uint32), (counts.ravel() & 0xFFFFFFFF).astype(np.uint32)) and not bool(hi.any())
    lo.copy_(torch.from_numpy((moved.ravel() & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).cuda())
    hi.copy_(torch.from_numpy((moved[:, 0] >> 32).astype(np.int32)).cuda())
    want = lab.copy()
    want[r:] = z
    dense = _dev_labels(want, lb)
    assert torch.equal(codes.to_dense().reshape(-1), dense)
    cen = (rng.randint(-8, 9, size=k) / 4.0).astype(np.float32)
    ct = _cuda(cen)
    for m in (7, 40):
        x, g = rng.randint(-3, 4, size=(m, kdim)).astype(np.float32), rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
        xt, gt = _half(x, dtype), _half(g, dtype)
        dc = _raw_dc(env, xt, gt, dtype, codes, True)
        assert _same(dc, ops.codebook_centroid_grad(xt, gt, dense, k, kdim, ncols)) and np.array_equal(dc.cpu().numpy(), ref.dc64(x, g, want, k))
        dx = _raw_dx(env, gt, dtype, codes, ct, False)
        assert np.array_equal(dx.cpu().numpy(), ref.dx64(g, want, cen).astype(np.float32))


# ------------------------------------------------------------------ 4. the ranges of the two types
@pytest.mark.parametrize("m", [5, 40])
def test_bf16_dc_across_the_exponent_range_and_both_sides_of_p127(env, m):
    """products near 2^-160 (the scaling of section 12 keeps them), and m max|x| max|g| on both sides of 2^127 (above: all NaN):
    the byte form's call bit for bit"""
    _, ops, _ = env
    kdim, ncols, k, z = 33, 65, 17, 2
    rng = np.random.RandomState(m)
    from tests.helpers.sparse_ref import labels_at_density
    lab = labels_at_density(rng, kdim, ncols, k, 0.3, z)
    codes, dense = _codes(env, lab, 1, k, z), _dev_labels(lab, 1)
    base_x, base_g = rng.randint(-3, 4, size=(m, kdim)).astype(np.float64), rng.randint(-3, 4, size=(m, ncols)).astype(np.float64)
    for ex, eg, nan in ((-80, -80, False), (-120, 10, False), (50, 50, False), (64, 62 - int(np.ceil(np.log2(m * 9))), False), (64, 63, True)):
        xt, gt = _half(base_x * 2.0 ** ex, "bf16"), _half(base_g * 2.0 ** eg, "bf16")
        for out in (torch.float64, torch.float32):
            dc = ops.sparse_codebook_centroid_grad(xt, gt, codes, dtype=out)
            assert _same_or_both_nan(dc, ops.codebook_centroid_grad(xt, gt, dense, k, kdim, ncols, dtype=out))
            assert bool(torch.isnan(dc).all()) == nan
            if not nan and out == torch.float64:
                assert np.array_equal(dc.cpu().numpy(), ref.dc64(base_x, base_g, lab, k) * 2.0 ** (ex + eg))


@pytest.mark.parametrize("m", [5, 40])
def test_fp16_extremes(env, m):
    """65504 next to subnormals in x and g, and a centre of 1e5 (Inf as fp16): the byte form's calls bit for bit"""
    _, ops, _ = env
    kdim, ncols, k, z = 33, 65, 17, 2
    rng = np.random.RandomState(m)
    from tests.helpers.sparse_ref import labels_at_density
    lab = labels_at_density(rng, kdim, ncols, k, 0.3, z)
    codes, dense = _codes(env, lab, 1, k, z), _dev_labels(lab, 1)
    x = rng.choice([65504.0, -65504.0, 2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -14, 1.0, 0.0], size=(m, kdim))
    g = rng.choice([65504.0, 2.0 ** -24, -2.0 ** -20, 1.0, 0.0], size=(m, ncols))
    xt, gt = _half(x, "fp16"), _half(g, "fp16")
    for out in (torch.float64, torch.float32):
        dc = ops.sparse_codebook_centroid_grad(xt, gt, codes, dtype=out)
        assert _same(dc, ops.codebook_centroid_grad(xt, gt, dense, k, kdim, ncols, dtype=out)) and bool(torch.isfinite(dc).all())
    cen = (rng.randint(-8, 9, size=k) / 4.0).astype(np.float32)
    cen[5] = 1e5
    ct = _cuda(cen)
    g1 = _half(rng.randint(-3, 4, size=(m, ncols)), "fp16")
    dx = ops.sparse_codebook_matmul_dx(g1, codes, ct, out_dtype=torch.float32)
    if m > 16:
        assert _same_or_both_nan(dx, ops.codebook_matmul_dx(g1, dense, ct, kdim, ncols, out_dtype=torch.float32))
    else:
        assert _same_or_both_nan(dx, ops.sparse_codebook_matmul_dx(g1.float(), codes, ct.half().float()))
    assert not bool(torch.isfinite(dx).all())


# ------------------------------------------------------------------ 5. ops.sparse_codebook_linear: no host read, dtypes, errors
def _exact_layer(m, kdim=90, ncols=150, k=40, seed=0, density=0.3):
    rng = np.random.RandomState(seed)
    from tests.helpers.sparse_ref import labels_at_density
    x = rng.randint(-3, 4, size=(m, kdim)).astype(np.float32)
    c = (rng.randint(-8, 9, size=k) / 4.0).astype(np.float32)
    lab = labels_at_density(rng, kdim, ncols, k, density, 1)
    b = rng.randint(-4, 5, size=ncols).astype(np.float32)
    return x, c, lab, b


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_forward_plus_backward_makes_no_host_read(env, dtype):
    _, ops, _ = env
    x, c, lab, b = _exact_layer(m=40)
    codes = ops.pack_sparse_codes(_dev_labels(lab, 1), 90, 150, 40, zero_symbol=1)
    ct, bt = _cuda(c).requires_grad_(True), _cuda(b).requires_grad_(True)
    xt, x5 = _half(x, dtype).requires_grad_(True), _half(x[:5], dtype).requires_grad_(True)
    gy, gy5 = _half(np.ones((40, 150)), dtype), _half(np.ones((5, 150)), dtype)
    ops.sparse_codebook_linear(xt, codes, ct, bias=bt, relu=True).backward(gy)       # (warm: allocations, the library load)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for relu in (False, True):
            y = ops.sparse_codebook_linear(xt, codes, ct, bias=bt, relu=relu)
            y.backward(gy)
            ops.sparse_codebook_linear(x5, codes, ct, bias=bt, relu=relu).backward(gy5)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert y.dtype == _tdt(dtype) and xt.grad.dtype == _tdt(dtype) and ct.grad.dtype == torch.float32 and bt.grad.dtype == torch.float32


def test_dtype_errors(env):
    _, ops, _ = env
    x, c, lab, b = _exact_layer(m=3)
    codes = ops.pack_sparse_codes(_dev_labels(lab, 1), 90, 150, 40, zero_symbol=1)
    ct, bt = _cuda(c), _cuda(b)
    g, xh = _half(np.ones((3, 150)), "bf16"), _half(x, "bf16")
    with pytest.raises(TypeError):
        ops.sparse_codebook_matmul_dx(g, codes, ct.bfloat16())
    with pytest.raises(TypeError):
        ops.sparse_codebook_matmul_dx(g, codes, ct, out_dtype=torch.float16)
    with pytest.raises(TypeError):
        ops.sparse_codebook_matmul_dx(g.float(), codes, ct, out_dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        ops.sparse_codebook_centroid_grad(xh, g.half(), codes)
    with pytest.raises(TypeError):
        ops.sparse_codebook_centroid_grad(xh.float(), g, codes)
    with pytest.raises(TypeError):
        ops.sparse_codebook_linear(xh, codes, ct.bfloat16())
    with pytest.raises(TypeError):
        ops.sparse_codebook_linear(xh, codes, ct, bias=bt.bfloat16())
    assert ops.sparse_codebook_matmul_dx(g, codes, ct).dtype == torch.bfloat16
    assert ops.sparse_codebook_matmul_dx(g.float(), codes, ct, out_dtype=torch.float32).dtype == torch.float32


# ------------------------------------------------------------------ 6. the layers
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", [None, torch.relu])
def test_sparse_and_byte_trainable_dense_agree_bit_for_bit(env, dtype, act):
    """m > 16: a TrainableSparseCompressedDense(half_inputs=True) and a TrainableCompressedDense(half_inputs=True) on to_dense() give
    the same output, x.grad, centers.grad and bias.grad, float data, with a fused ReLU too"""
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    rng = np.random.RandomState(3)
    kdim, ncols, k, m = 129, 200, 40, 40
    from tests.helpers.sparse_ref import labels_at_density
    lab = labels_at_density(rng, kdim, ncols, k, 0.3, 4)
    labels, ct, bt = _dev_labels(lab, 1), _cuda((rng.randn(k) * 0.1).astype(np.float32)), _cuda(rng.randn(ncols).astype(np.float32))
    codes = ops.pack_sparse_codes(labels, kdim, ncols, k)
    sparse = compressed.TrainableSparseCompressedDense(codes, labels, ct, bt, None, act, half_inputs=True)
    byte = compressed.TrainableCompressedDense(kdim, ncols, codes.to_dense(), ct, bt, None, act, half_inputs=True)
    assert sparse.half_inputs and torch.equal(sparse.kernel_sq_sum(), byte.kernel_sq_sum())
    x = rng.randn(m, kdim)
    gy = _half(rng.randn(m, ncols) * 0.01, dtype)
    outs = []
    for layer in (sparse, byte):
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
def test_trainable_sparse_conv_with_half_inputs(env, dtype, ks, cin, cout, pad, hw):
    """exact data: the layer's output and centre gradient are the float64 formulas on the patches"""
    from neural_network_compression_amd import compressed

    rng = np.random.RandomState(ks)
    k, kdim = 9, ks * ks * cin
    lab = rng.randint(0, k, size=kdim * cout).astype(np.uint8)
    lab[rng.rand(lab.size) < 0.6] = 2
    c = (rng.randint(-4, 5, size=k) / 4.0).astype(np.float32)
    lab_t = _cuda(lab)
    lab_u = compressed._unfold_labels(ks, cin, cout, lab_t)
    codes = compressed._unfold_then_pack(compressed.ops.pack_sparse_codes, ks, cin, cout, lab_t, k, None)
    layer = compressed.TrainableSparseCompressedConv2D(ks, cin, pad, codes, lab_t, _cuda(c), None, None, None, half_inputs=True)
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
    with pytest.raises(TypeError, match="byte form"):
        compressed.TrainableSparseCompressedConv2D(ks, cin, pad, codes, lab_t, _cuda(c))(xt.detach())


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
        lt = _dev_labels(lab, 1)
        layers.append(compressed.TrainableSparseCompressedDense(ops.pack_sparse_codes(lt, kd, nc, c.size), lt, _cuda(c), half_inputs=True))
    out = layers[1](layers[0](_half(x, dtype)))
    assert np.array_equal(out.detach().float().cpu().numpy(), y.detach().numpy())
    out.backward(_half(gy, dtype))
    for layer, w, lab, k in ((layers[0], w1, lab1, 5), (layers[1], w2, lab2, 3)):
        assert np.array_equal(layer.centers.grad.cpu().numpy(), ref.bin64(w.grad.numpy(), lab, k).astype(np.float32))


def test_without_the_option_half_inputs_raise_and_float32_keeps_its_bits(env):
    """Plain layers still raise TypeError ("byte form") on a half input.  A float32 input through every sparse trainable layer, built
    either way, gives the bits of nnc_cbsp_dx_f32 / nnc_cbsp_dc_f32 called directly."""
    from neural_network_compression_amd import compressed

    L, ops, _ = env
    rng = np.random.RandomState(11)
    kdim, ncols, k = 129, 100, 30
    from tests.helpers.sparse_ref import labels_at_density
    lab = labels_at_density(rng, kdim, ncols, k, 0.3, 0)
    labels, ct = _dev_labels(lab, 1), _cuda((rng.randn(k) * 0.1).astype(np.float32))
    codes = ops.pack_sparse_codes(labels, kdim, ncols, k)
    stream = torch.cuda.current_stream().cuda_stream

    def direct(x, g):
        m = x.shape[0]
        dx, dc = torch.empty(m, kdim, device="cuda"), torch.empty(k, device="cuda")
        nb = int(L.nnc_cbsp_dx_workspace_bytes(m, kdim, ncols, 1))
        ws = torch.empty(max(nb, 8), dtype=torch.uint8, device="cuda")
        ops.nat.check(L.nnc_cbsp_dx_f32(g.data_ptr(), m, kdim, codes.buf.data_ptr(), codes.nbytes(), 1, ncols, codes.zero_symbol, codes.nnz, ct.data_ptr(), k,
                                        dx.data_ptr(), ws.data_ptr() if nb else None, nb, stream))
        nb = int(L.nnc_cbsp_dc_workspace_bytes(m, kdim, ncols, 1, k))
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        ops.nat.check(L.nnc_cbsp_dc_f32(x.data_ptr(), g.data_ptr(), m, kdim, codes.buf.data_ptr(), codes.nbytes(), 1, ncols, codes.zero_symbol, codes.nnz, k,
                                        dc.data_ptr(), 0, ws.data_ptr(), nb, stream))
        return dx, dc

    built = [compressed.TrainableSparseCompressedDense.from_codes(kdim, ncols, labels, ct),
             compressed.TrainableSparseCompressedDense(codes, labels, ct),
             compressed.TrainableSparseCompressedDense(codes, labels, ct, half_inputs=True)]
    assert [b.half_inputs for b in built] == [False, False, True]
    for m in (7, 40):
        x, g = torch.randn(m, kdim, device="cuda"), torch.randn(m, ncols, device="cuda") * 0.01
        dx, dc = direct(x, g)
        for layer in built:
            layer.centers.grad = None
            xt = x.clone().requires_grad_(True)
            layer(xt).backward(g)
            assert _same(xt.grad, dx) and _same(layer.centers.grad, dc)
    for tdt in (torch.bfloat16, torch.float16):
        for layer in built[:2]:
            with pytest.raises(TypeError, match="byte form"):
                layer(torch.zeros(3, kdim, dtype=tdt, device="cuda"))
        assert built[2](torch.zeros(3, kdim, dtype=tdt, device="cuda")).dtype == tdt
    conv_lab = _cuda(rng.randint(0, 9, size=3 * 3 * 2 * 4).astype(np.uint8))
    conv = compressed.TrainableSparseCompressedConv2D.from_codes(3, 2, 4, 1, conv_lab, _cuda(np.linspace(-1, 1, 9).astype(np.float32)))
    with pytest.raises(TypeError, match="byte form"):
        conv(torch.zeros(2, 6, 6, 2, dtype=torch.bfloat16, device="cuda"))


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


def test_one_batch_of_fine_tune_compressed_sparse_in_bf16_is_the_step_from_the_ops_calls(env, quantized):
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    t, tr, data, test = quantized
    models = t.quantized_models_by_layer
    dt, lr = torch.bfloat16, 1e-2
    c0 = _centres(models)
    names = ("dense1", "dense2", "out")
    layers = [getattr(t.neural_network, n) for n in names]
    net = compressed.compress_network_trainable(t.neural_network, models, sparse=True, sparse_half_inputs=True)
    assert all(isinstance(l, compressed.TrainableSparseCompressedDense) and l.half_inputs for l in net.get_config().values())
    auto = compressed.compress_network_trainable(t.neural_network, models, sparse="auto", sparse_half_inputs=True)
    plain = compressed.compress_network_trainable(t.neural_network, models, sparse="auto")
    assert [type(a) for a in auto.get_config().values()] == [type(p) for p in plain.get_config().values()]      # what "auto" picks does not change
    assert all(l.half_inputs for l in auto.get_config().values())
    # the step from the ops calls, on the batch fine_tune_compressed will draw
    torch.manual_seed(5)
    xb, yb = next(tr._batches(t._to_device(data.input_data).float(), t._to_device(data.output_data).float()))
    cs = [torch.from_numpy(c0[(l, 0)]).cuda() for l in layers]
    bcs = [torch.from_numpy(c0[(l, 1)]).cuda() if (l, 1) in c0 else None for l in layers]
    labs = [models[l][0].labels_compact_ for l in layers]
    blabs = [models[l][1].labels_compact_ if (l, 1) in c0 else None for l in layers]
    biases = [ops.gather(bcs[i], blabs[i]) if bcs[i] is not None else layers[i].bias.detach() for i in range(3)]
    shapes = [tuple(l.kernel.shape) for l in layers]
    codes = [ops.pack_sparse_codes(labs[i], *shapes[i], cs[i].numel()) for i in range(3)]
    acts = [xb.to(dt)]
    with torch.no_grad():
        for i in range(3):
            acts.append(ops.sparse_codebook_matmul(acts[-1], codes[i], cs[i], bias=biases[i], relu=i < 2))
    logits = acts[-1].float().requires_grad_(True)
    torch.nn.functional.binary_cross_entropy_with_logits(logits, yb).backward()
    g = logits.grad.to(dt)
    want = {}
    for i in (2, 1, 0):
        if i < 2:
            g = torch.where(acts[i + 1] > 0, g, torch.zeros((), dtype=dt, device="cuda"))
        dc = ops.sparse_codebook_centroid_grad(acts[i], g, codes[i], dtype=torch.float32)
        assert torch.equal(dc, ops.codebook_centroid_grad(acts[i], g, labs[i], cs[i].numel(), *shapes[i], dtype=torch.float32))
        cp = cs[i].clone().requires_grad_(True)
        counts = ops.bincount(labs[i], cs[i].numel())
        (0.01 * ((counts.to(torch.float32) * cp ** 2).sum() / 2)).backward()
        want[(layers[i], 0)] = (cs[i], dc, cp.grad)
        if bcs[i] is not None:
            db = ops.centroid_gradient(g.sum(0, dtype=torch.float32).contiguous(), blabs[i], bcs[i].numel()).to(torch.float32)
            want[(layers[i], 1)] = (bcs[i], db, None)
        if i > 0:
            g = ops.sparse_codebook_matmul_dx(g, codes[i], cs[i])

    kw = dict(sparse=True, activation_dtype=dt, sparse_half_inputs=True)
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


def test_fine_tune_compressed_sparse_half_errors(env, quantized):
    t, tr, data, test = quantized
    for kw in (dict(sparse=True), dict(sparse="auto")):                                  # pinned: without the new keyword
        with pytest.raises(ValueError):
            t.fine_tune_compressed(data, test, epochs=1, activation_dtype=torch.bfloat16, **kw)
    with pytest.raises(ValueError, match="sparse_half_inputs"):
        t.fine_tune_compressed(data, test, epochs=1, sparse=True, sparse_half_inputs=True)
    with pytest.raises(ValueError, match="sparse_half_inputs"):
        t.fine_tune_compressed(data, test, epochs=1, activation_dtype=torch.bfloat16, sparse_half_inputs=True)
    with pytest.raises(ValueError):
        t.compressed_network(trainable=True, half_inputs=True, sparse=True)
    models = t.quantized_models_by_layer
    kept = models[t.neural_network.dense2]
    models[t.neural_network.dense2] = [None, None]              # dense2 passed through unquantized
    try:
        with pytest.raises(ValueError, match="dense2"):
            t.fine_tune_compressed(data, test, epochs=1, sparse=True, activation_dtype=torch.float16, sparse_half_inputs=True)
    finally:
        models[t.neural_network.dense2] = kept
