"""The group-wise codebook matmul on 2- and 4-bit packed indices (nnc_cbpk_grouped, csrc/nnc_cbpk_grouped.hip)
against float64 NumPy, through the raw C ABI with buffers the test owns, and through ops.grouped_packed_codebook_matmul,
GroupedPackedCompressedDense and pack_grouped_layers (run with -m gpu).

Every case of tests/helpers/grouped_packed_ref.py with float32, bf16 and fp16 activations: exact data bit for bit (float32 output,
with and without ReLU; half output = that result rounded once; the bits of ops.grouped_codebook_matmul on the unpacked labels),
float data within the bounds of the byte-form grouped test, every call into sentinel-framed y and workspace slices and repeated
for the same bits.  Then one group against ops.packed_codebook_matmul bit for bit, the rows on both sides of every boundary picked
out by one-hot and identity x, non-finite inputs and indices >= K, degenerate shapes, the op's and the layer's rules, and
pack_grouped_layers on a fitted network.

The float bounds are those of tests/test_gpu_grouped_codebook.py.  float32 x: 2 kdim 2^-24 (|x| @ |W| + |bias|).  Half x: the
products are exact, so (kdim + splits + 2) 2^-23 mag with mag = |x| @ |W_h| + |bias|, plus half an ulp of the dtype at |ref| for a
half output."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import cbmm_ref, grouped_packed_ref as gp, grouped_ref, h16_ref, packed_ref  # noqa: E402
from tests.helpers.cbmm_ref import relu_like_torch  # noqa: E402
from tests.helpers.grouped_packed_ref import CASES, DTYPES  # noqa: E402

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
    return gp.torch_dtype(dtype)


def _round(values, dtype):
    return np.asarray(values, dtype=np.float32) if dtype == "f32" else h16_ref.round_to(values, dtype)


def _dev(host, tdtype, view=False):
    """host float32 values -> device tensor of ``tdtype``; ``view``: as buf[1:] of a one-longer buffer (aligned to the element
    size and no further)."""
    t = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).to(tdtype)
    if not view:
        return t.cuda()
    buf = torch.zeros(t.numel() + 1, dtype=tdtype, device="cuda")
    buf[1:] = t.reshape(-1).cuda()
    return buf[1:].view(t.shape)


def _dev_packed(lab, kdim, ncols, bits):
    """The labels in the layout of include/nnc.h, packed on the host (packed_ref.pack), as a device buffer (16-byte aligned)."""
    t = torch.from_numpy(packed_ref.pack(lab, kdim, ncols, bits)).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _dev_labels(lab):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(lab).ravel().astype(np.uint8))).cuda()


def _call(env, x, dtype, m, kdim, packed, bits, ncols, centers, k, group_rows, bias, relu, half_out):
    """nnc_cbpk_grouped into sentinel-framed y and workspace (exactly the queried size); checks the frames; returns y as float32
    (device, m x ncols) and its raw bits.  A half y starts an odd number of 2-byte units into its buffer, a float32 y on a 4-byte
    boundary that is no 8-byte one."""
    L, ops, _ = env
    dt = gp.DT_CODE[dtype]
    assert not (half_out and dtype == "f32")
    ws_bytes = int(L.nnc_cbpk_grouped_workspace_bytes(dt, m, kdim, ncols, bits))
    assert ws_bytes % 4 == 0
    mn = m * ncols
    units, pad = (mn, 37) if half_out else (2 * mn, 38)
    ybuf = torch.full((units + 2 * pad,), SENT16, dtype=torch.int16, device="cuda")
    wsbuf = torch.full((ws_bytes // 4 + 2 * WS_PAD,), SENT32, dtype=torch.int32, device="cuda")
    y = ybuf[pad: pad + units]
    ws_ptr = wsbuf[WS_PAD:].data_ptr() if ws_bytes else None
    ops.nat.check(L.nnc_cbpk_grouped(x.data_ptr(), dt, m, kdim, packed.data_ptr(), packed.numel(), bits, ncols, centers.data_ptr(), k, group_rows,
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


def _plan(env, c, dtype):
    _, ops, cus = env
    return ops.cbpk_grouped_plan(_tdt(dtype), c["m"], c["kdim"], c["ncols"], c["bits"], c["k"], c["group_rows"], cus)


# ------------------------------------------------------------------ the regimes at this device
def test_the_cases_hit_every_regime_at_this_device(env):
    hit, walks = set(), {}
    for c in CASES:
        for dtype in DTYPES:
            p = _plan(env, c, dtype)
            r = gp.regime_of(c, p, dtype)
            hit.add(r)
            walks.setdefault(r[0], set()).update(gp.walks_of(c, p))
    assert hit == gp.required_regimes(), sorted(gp.required_regimes() - hit)
    for kernel in ("stream", "tiled", "mfma"):
        assert gp.required_walks(kernel) <= walks[kernel], (kernel, walks[kernel])
    _, ops, cus = env
    p = ops.cbpk_grouped_plan(torch.float32, 1, 112, 70, 2, 3, 32, cus)
    assert (p["splits"], p["rps"]) == (3, 38), p                      # splits that start at rows 38 and 76, inside groups 1 and 2
    p = ops.cbpk_grouped_plan(torch.float32, 17, 300, 50, 4, 16, 32, cus)
    assert (p["path"], p["splits"], p["rps"]) == (gp.PATH_TILED, 2, 150), p   # the step of rows 158..165 lies across row 160
    p = ops.cbpk_grouped_plan(torch.bfloat16, 17, 300, 50, 4, 16, 32, cus)
    assert (p["path"], p["splits"], p["rps"]) == (gp.PATH_MFMA, 4, 96), p


# ------------------------------------------------------------------ every case: exact data, float data, frames, the same bits
@pytest.fixture(scope="module")
def case_data():
    """Per case, made once: labels, exact data and float data on the host (the float64 references are formed per dtype)."""
    out = []
    for ci, c in enumerate(CASES):
        lab, x, cen, bias = grouped_ref.exact_data(c, 9000 + ci)
        xf, cf, bf = grouped_ref.float_data(c, 9000 + ci)
        out.append(dict(lab=lab, x=x, cen=cen, bias=bias, xf=xf, cf=cf, bf=bf))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[gp.case_id(c) for c in CASES])
def test_case(env, case_data, ci, dtype):
    _, ops, _ = env
    c, d = CASES[ci], case_data[ci]
    m, kdim, ncols, k, rows, bits = c["m"], c["kdim"], c["ncols"], c["k"], c["group_rows"], c["bits"]
    tdt = _tdt(dtype)
    halves = (False,) if dtype == "f32" else (False, True)
    pk_t, lab_t = _dev_packed(d["lab"], kdim, ncols, bits), _dev_labels(d["lab"])
    codes = ops.pack_codes(lab_t, kdim, ncols, k)
    assert codes.bits == bits and torch.equal(codes.packed, pk_t)        # the device's pack pass writes the layout the host reference writes
    p = _plan(env, c, dtype)

    # exact data: the float64 result bit for bit; the half output is that result rounded once; the same bits a second time; the
    # bits of the byte-form grouped call on the unpacked labels
    x, cen, bias = d["x"], d["cen"], d["bias"]
    w = grouped_ref.weights(cen, d["lab"], kdim, ncols, rows, dtype)
    cbmm_ref.assert_exact(x, w, bias)
    want = grouped_ref.reference(x, w, bias)
    x_t, cen_t = _dev(x, tdt, c["x_view"]), _dev(cen, torch.float32)
    bias_t = None if bias is None else _dev(bias, torch.float32, c["bias_view"])
    last = {}
    for relu in (False, True):
        ref = (relu_like_torch(want) if relu else want).astype(np.float32)
        for half_out in halves:
            y, ybits = _call(env, x_t, dtype, m, kdim, pk_t, bits, ncols, cen_t, k, rows, bias_t, relu, half_out)
            r = _round(ref, dtype) if half_out else ref
            got = y.cpu().numpy()
            assert np.array_equal(got, r), (c, relu, half_out, np.argwhere(got != r)[:5])
            byte = ops.grouped_codebook_matmul(x_t, codes.to_dense(), cen_t, kdim, ncols, rows, bias=bias_t, relu=relu,
                                               out_dtype=None if half_out or dtype == "f32" else torch.float32)
            assert torch.equal(byte.reshape(-1).view(torch.int16), ybits), (c, relu, half_out)
            last[half_out] = ybits
    for half_out in halves:
        assert torch.equal(last[half_out], _call(env, x_t, dtype, m, kdim, pk_t, bits, ncols, cen_t, k, rows, bias_t, True, half_out)[1])

    # float data: x rounded to the dtype, arbitrary float32 centres (rounded by the kernel as centers.to(dtype)), float32 bias
    xf = _round(d["xf"], dtype)
    wf = grouped_ref.weights(d["cf"], d["lab"], kdim, ncols, rows, dtype)
    bf = d["bf"]
    ref = grouped_ref.reference(xf, wf, bf)
    mag = np.abs(xf.astype(np.float64)) @ np.abs(wf.astype(np.float64)) + (0 if bf is None else np.abs(bf.astype(np.float64)))
    bound = 2 * kdim * 2.0 ** -24 * mag if dtype == "f32" else (kdim + p["splits"] + 2) * 2.0 ** -23 * mag
    xf_t, cf_t = _dev(xf, tdt, c["x_view"]), _dev(d["cf"], torch.float32)
    bf_t = None if bf is None else _dev(bf, torch.float32, c["bias_view"])
    for half_out in halves:
        y, ybits = _call(env, xf_t, dtype, m, kdim, pk_t, bits, ncols, cf_t, k, rows, bf_t, False, half_out)
        err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
        b = bound + h16_ref.half_ulp(ref, dtype) if half_out else bound
        worst = float((err / np.maximum(b, 1e-300)).max())
        print(f"grouped packed float data: {gp.case_id(c)} {dtype} half_out={half_out}: largest err / bound = {worst:.4f}")
        assert np.all(err <= b), (c, dtype, half_out, worst)
        assert torch.equal(ybits, _call(env, xf_t, dtype, m, kdim, pk_t, bits, ncols, cf_t, k, rows, bf_t, False, half_out)[1])


# ------------------------------------------------------------------ the MFMA tile: the packed and the byte form share it
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_mfma_tile_gives_the_byte_forms_bits_on_float_data(env, case_data, dtype):
    """Half x at m > 16: nnc_cbpk_grouped and nnc_cbmm_grouped take the same grid (cb_grid), the same rounded table values and the
    same 128 x 128 MFMA tile (csrc/nnc_cbmfma.hpp), so on float data (grouped_ref.float_data) too, not only on exact data,
    ops.grouped_packed_codebook_matmul on the packed labels gives the bits of ops.grouped_codebook_matmul on the unpacked ones:
    every case whose plan here is the MFMA tile, half and float32 output, with and without ReLU."""
    _, ops, cus = env
    tdt = _tdt(dtype)
    ran = set()
    for c, d in zip(CASES, case_data):
        m, kdim, ncols, k, rows = c["m"], c["kdim"], c["ncols"], c["k"], c["group_rows"]
        p = _plan(env, c, dtype)
        if p["path"] != gp.PATH_MFMA:
            continue
        pb = ops.cbmm_grouped_plan(tdt, m, kdim, ncols, k, rows, cus)
        assert (pb["path"], pb["splits"], pb["rps"]) == (gp.PATH_MFMA, p["splits"], p["rps"]), (c, p, pb)
        lab_t = _dev_labels(d["lab"])
        codes = ops.pack_codes(lab_t, kdim, ncols, k)
        x_t, cen_t = _dev(_round(d["xf"], dtype), tdt, c["x_view"]), _dev(d["cf"], torch.float32)
        bias_t = None if d["bf"] is None else _dev(d["bf"], torch.float32, c["bias_view"])
        for out_dtype in (None, torch.float32):
            for relu in (False, True):
                got = ops.grouped_packed_codebook_matmul(x_t, codes, cen_t, rows, bias=bias_t, relu=relu, out_dtype=out_dtype)
                want = ops.grouped_codebook_matmul(x_t, lab_t, cen_t, kdim, ncols, rows, bias=bias_t, relu=relu, out_dtype=out_dtype)
                assert got.dtype == want.dtype == (tdt if out_dtype is None else torch.float32) and got.shape == want.shape == (m, ncols)
                assert torch.equal(got.reshape(-1).view(torch.int16), want.reshape(-1).view(torch.int16)), (c, dtype, out_dtype, relu)
        ran.add((c["bits"], "split" if p["splits"] > 1 else "direct"))
    assert ran == {(2, "direct"), (2, "split"), (4, "direct"), (4, "split")}, sorted(ran)


# ------------------------------------------------------------------ one group is the ungrouped packed call
def test_one_group_equals_packed_codebook_matmul(env):
    """group_rows >= kdim, float32, on every case of packed_ref.PACKED_REGIME_CASES, float data, bias, ReLU, x and bias as views:
    ops.packed_codebook_matmul's bits."""
    _, ops, _ = env
    for ci, c in enumerate(packed_ref.PACKED_REGIME_CASES):
        m, kdim, ncols, k, bits = c["m"], c["kdim"], c["ncols"], c["k"], c["bits"]
        rng = np.random.RandomState(300 + ci)
        codes = ops.pack_codes(_dev_labels(rng.randint(0, k, size=kdim * ncols)), kdim, ncols, k, bits)
        cen_t = torch.from_numpy(rng.standard_normal(k).astype(np.float32)).cuda()
        bias_t = _dev(rng.standard_normal(ncols), torch.float32, c["bias_view"]) if c["bias"] else None
        x_t = _dev(rng.standard_normal((m, kdim)), torch.float32, c["x_view"])
        rows = -(-kdim // 32) * 32 + 32 * (ci % 3)                      # group_rows >= kdim: kdim rounded up, and beyond
        for relu in (False, True):
            want = ops.packed_codebook_matmul(x_t, codes, cen_t, bias=bias_t, relu=relu)
            got = ops.grouped_packed_codebook_matmul(x_t, codes, cen_t.view(1, k), rows, bias=bias_t, relu=relu)
            assert got.dtype == want.dtype and torch.equal(got.view(torch.int32), want.view(torch.int32)), (c, relu)


# ------------------------------------------------------------------ the rows beside every boundary
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kdim,ncols,k,rows", [(112, 70, 16, 32), (300, 50, 4, 32), (160, 130, 3, 64)])
def test_one_hot_and_identity_x_return_the_rows_of_w(env, dtype, kdim, ncols, k, rows):
    """x = the one-hot rows that select W's rows g R - 1 and g R (m <= 16: the stream kernel, in chunks) and x = I (m = kdim: the
    tiled kernel / the MFMA tile): y is those rows of W exactly, each from its own group's table (the centres are offset by 64 g)."""
    bits = gp.bits_of(k)
    c = dict(m=1, kdim=kdim, ncols=ncols, k=k, group_rows=rows, bias=False)
    lab, _, cen, _ = grouped_ref.exact_data(c, kdim)
    w = grouped_ref.weights(cen, lab, kdim, ncols, rows, dtype)
    pk_t, cen_t = _dev_packed(lab, kdim, ncols, bits), _dev(cen, torch.float32)
    picks = sorted({r for g in range(1, -(-kdim // rows)) for r in (g * rows - 1, g * rows)} | {0, kdim - 1})
    halves = (False,) if dtype == "f32" else (False, True)
    for lo in range(0, len(picks), 6):
        sel = picks[lo: lo + 6]
        x_t = _dev(np.eye(kdim, dtype=np.float32)[sel], _tdt(dtype))
        for half_out in halves:
            y, _ = _call(env, x_t, dtype, len(sel), kdim, pk_t, bits, ncols, cen_t, k, rows, None, False, half_out)
            assert np.array_equal(y.cpu().numpy(), w[sel]), (sel, half_out)
    x_t = _dev(np.eye(kdim, dtype=np.float32), _tdt(dtype))
    for half_out in halves:
        y, _ = _call(env, x_t, dtype, kdim, kdim, pk_t, bits, ncols, cen_t, k, rows, None, False, half_out)
        got = y.cpu().numpy()
        assert np.array_equal(got, w), (half_out, np.argwhere(got != w)[:5])


# ------------------------------------------------------------------ non-finite inputs, indices >= K
# (m, kdim, ncols, k, path for float32 x, path for half x, split): every kernel, direct and through the split-K combine; K = 5 at 4
# bits and K = 3 at 2 bits leave labels >= K that the width can hold
NONFINITE = [(8, 112, 77, 5, 1, 1, False), (3, 112, 70, 3, 1, 1, True), (17, 112, 130, 5, 2, 5, False), (17, 300, 50, 3, 2, 5, True)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,kdim,ncols,k,path32,path16,split", NONFINITE)
def test_nonfinite_inputs_propagate_and_an_index_past_k_reads_zero(env, dtype, m, kdim, ncols, k, path32, path16, split):
    """NaN and +-Inf in x, NaN in the bias; Inf against a centre that is exactly 0 gives NaN; a label >= K but < 2^bits reads 0 in
    every group (and Inf against it NaN).  The result equals the float64 one (NaN where it is NaN) and the byte-form grouped call's
    on the same labels; the fused ReLU maps -Inf to 0 and keeps NaN."""
    _, ops, cus = env
    rows, bits = 32, gp.bits_of(k)
    top = (1 << bits) - 1
    assert k <= top
    c = dict(m=m, kdim=kdim, ncols=ncols, k=k, group_rows=rows, bias=True)
    lab, x, cen, bias = grouped_ref.exact_data(c, m * 1000 + kdim)
    lab = lab.reshape(kdim, ncols)
    cen[:, 0] = 0.0
    lab[34, ::3] = 0                        # row 34 (group 1) meets +Inf against the exact 0 centre in every third column,
    lab[34, 1::3] = top                     # against a label >= K in the next ones;
    lab[9, :] = top                         # rows of labels >= K in groups 0 and 2
    lab[70, :] = k
    x[0, 1] = np.nan
    x[1, 34] = np.inf                       # +Inf where W[34] > 0, NaN against the 0 centre and the label >= K
    x[2, 64] = -np.inf                      # group 2's centres are positive: -Inf
    if m > 3:
        x[m - 1, kdim - 1] = np.inf
        x[m - 1, 5] = -np.inf
    bias[4] = np.nan
    w = grouped_ref.weights(cen, lab, kdim, ncols, rows, dtype)
    assert np.all(w[9] == 0) and np.all(w[70] == 0)
    cbmm_ref.assert_exact(np.where(np.isfinite(x), x, 0), w, np.where(np.isfinite(bias), bias, 0))
    pk_t, lab_t = _dev_packed(lab, kdim, ncols, bits), _dev_labels(lab)
    p = ops.cbpk_grouped_plan(_tdt(dtype), m, kdim, ncols, bits, k, rows, cus)
    assert p["path"] == (path32 if dtype == "f32" else path16) and (p["splits"] > 1) == split, p
    want = grouped_ref.reference(x, w, bias)
    assert np.isnan(want).any() and np.isposinf(want).any() and np.isneginf(want).any()
    x_t, cen_t, bias_t = _dev(x, _tdt(dtype)), _dev(cen, torch.float32), _dev(bias, torch.float32)
    for relu in (False, True):
        ref = (relu_like_torch(want) if relu else want).astype(np.float32)
        for half_out in ((False,) if dtype == "f32" else (False, True)):
            y = _call(env, x_t, dtype, m, kdim, pk_t, bits, ncols, cen_t, k, rows, bias_t, relu, half_out)[0].cpu().numpy()
            r = _round(ref, dtype) if half_out else ref
            assert np.array_equal(y, r, equal_nan=True), (relu, half_out, np.argwhere(~((y == r) | (np.isnan(y) & np.isnan(r))))[:5])
            byte = ops.grouped_codebook_matmul(x_t, lab_t, cen_t, kdim, ncols, rows, bias=bias_t, relu=relu,
                                               out_dtype=None if half_out or dtype == "f32" else torch.float32).float().cpu().numpy()
            assert np.array_equal(y, byte, equal_nan=True), (relu, half_out)


def test_degenerate_shapes(env):
    """m = 0 and ncols = 0 write nothing; kdim = 0 writes the bias (with and without ReLU), in float32 and in half."""
    _, ops, _ = env
    cen_t = torch.ones(1, 4, device="cuda")
    empty = torch.zeros(16, dtype=torch.uint8, device="cuda")[:0]
    bias = np.array([-1.5, 2.25, 0.0, 1000.0, -3.0], dtype=np.float32)
    bias_t = torch.from_numpy(bias).cuda()
    lab40 = torch.zeros(40 * 5, dtype=torch.uint8, device="cuda")
    for dtype in DTYPES:
        x_t = torch.zeros(8, dtype=_tdt(dtype), device="cuda")
        for half_out in ((False,) if dtype == "f32" else (False, True)):
            for bits in (2, 4):
                for relu in (False, True):
                    y, _ = _call(env, x_t, dtype, 3, 0, empty, bits, 5, cen_t, 4, 32, bias_t, relu, half_out)
                    assert np.array_equal(y.cpu().numpy(), np.tile(np.maximum(bias, 0) if relu else bias, (3, 1)))
        x2 = torch.zeros((0, 40), dtype=_tdt(dtype), device="cuda")
        cen2 = torch.ones(2, 4, device="cuda")
        assert ops.grouped_packed_codebook_matmul(x2, ops.pack_codes(lab40, 40, 5, 4), cen2, 32).shape == (0, 5)
        assert ops.grouped_packed_codebook_matmul(x_t.view(1, 8), ops.pack_codes(lab40[:0], 8, 0, 4), cen_t, 32).shape == (1, 0)


# ------------------------------------------------------------------ ops and the layer
def _layer_data(rng, kdim, ncols, k, rows):
    c = dict(m=1, kdim=kdim, ncols=ncols, k=k, group_rows=rows, bias=True)
    lab, _, cen, bias = grouped_ref.exact_data(c, rng.randint(1 << 20))
    return torch.from_numpy(lab.astype(np.uint8)).cuda(), torch.from_numpy(cen).cuda(), torch.from_numpy(bias).cuda()


def test_ops_argument_and_dtype_rules(env):
    _, ops, _ = env
    kdim, ncols, k, rows = 112, 70, 16, 32
    lab_t, cen_t, bias_t = _layer_data(np.random.RandomState(1), kdim, ncols, k, rows)
    codes = ops.pack_codes(lab_t, kdim, ncols, k)
    x = torch.from_numpy(np.random.RandomState(2).randint(-4, 5, size=(2, 5, kdim)).astype(np.float32)).cuda()
    y32 = ops.grouped_packed_codebook_matmul(x, codes, cen_t, rows, bias=bias_t)
    assert y32.shape == (2, 5, ncols) and y32.dtype == torch.float32
    w = grouped_ref.weights(cen_t.cpu().numpy(), lab_t.cpu().numpy(), kdim, ncols, rows)
    assert np.array_equal(y32.cpu().numpy().reshape(10, ncols), (grouped_ref.reference(x.cpu().numpy().reshape(10, kdim), w, bias_t.cpu().numpy())).astype(np.float32))
    for tdt in (torch.bfloat16, torch.float16):
        yf = ops.grouped_packed_codebook_matmul(x.to(tdt), codes, cen_t, rows, bias=bias_t, out_dtype=torch.float32)
        yh = ops.grouped_packed_codebook_matmul(x.to(tdt), codes, cen_t, rows, bias=bias_t)
        assert yf.dtype == torch.float32 and yh.dtype == tdt and torch.equal(yh, yf.to(tdt))
        with pytest.raises(TypeError):
            ops.grouped_packed_codebook_matmul(x.to(tdt), codes, cen_t, rows, out_dtype=torch.float64)
        with pytest.raises(TypeError):
            ops.grouped_packed_codebook_matmul(x.to(tdt), codes, cen_t.to(tdt), rows)
        with pytest.raises(RuntimeError, match="inference only"):
            ops.grouped_packed_codebook_matmul(x.to(tdt).requires_grad_(), codes, cen_t, rows)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.grouped_packed_codebook_matmul(x.clone().requires_grad_(), codes, cen_t, rows)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.grouped_packed_codebook_matmul(x, codes, cen_t.clone().requires_grad_(), rows)
    with torch.no_grad():
        assert torch.equal(ops.grouped_packed_codebook_matmul(x.clone().requires_grad_(), codes, cen_t, rows, bias=bias_t), y32)
    with pytest.raises(TypeError):
        ops.grouped_packed_codebook_matmul(x.double(), codes, cen_t, rows)
    with pytest.raises(TypeError, match="PackedCodes"):                  # the byte labels are not a packed form
        ops.grouped_packed_codebook_matmul(x, lab_t, cen_t, rows)
    for bad_rows in (0, 16, 48, -32):
        with pytest.raises(ValueError, match="group_rows"):
            ops.grouped_packed_codebook_matmul(x, codes, cen_t, bad_rows)
    with pytest.raises(ValueError, match="centers"):                     # 4 groups need 4 codebooks
        ops.grouped_packed_codebook_matmul(x, codes, cen_t[:3].contiguous(), rows)
    with pytest.raises(ValueError, match="centers"):
        ops.grouped_packed_codebook_matmul(x, codes, cen_t.reshape(-1), rows)
    with pytest.raises(ValueError, match="centers"):                     # K is the codes' K
        ops.grouped_packed_codebook_matmul(x, codes, cen_t[:, :15].contiguous(), rows)
    with pytest.raises(ValueError):                                      # K > 16 has no packed form
        ops.pack_codes(lab_t, kdim, ncols, 17)


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16, torch.float16])
def test_layer_matches_the_op_and_a_chain_stays_in_its_dtype(env, tdt):
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    kdim, ncols, k, rows = 300, 100, 16, 64
    rng = np.random.RandomState(3)
    lab1, cen1, bias1 = _layer_data(rng, kdim, ncols, k, rows)
    lab2, cen2, _ = _layer_data(rng, ncols, kdim, 4, 32)
    l1 = compressed.GroupedPackedCompressedDense.from_codes(kdim, ncols, rows, lab1, cen1, bias1, torch.relu)
    l2 = compressed.GroupedPackedCompressedDense.from_codes(ncols, kdim, 32, lab2, cen2 / 64, None, torch.tanh)
    assert (l1.bits, l2.bits) == (4, 2)
    assert l1.nbytes() == kdim * packed_ref.row_bytes(ncols, 4) + 4 * 5 * k + 4 * ncols == compressed.compressed_nbytes(l1)
    assert l2.nbytes() == ncols * packed_ref.row_bytes(kdim, 2) + 4 * 4 * 4
    assert l1.get_weights() == []
    c1, c2 = ops.pack_codes(lab1, kdim, ncols, k), ops.pack_codes(lab2, ncols, kdim, 4)
    for m in (1, 5, 40):
        x = torch.randn(m, kdim, device="cuda").to(tdt)
        with torch.no_grad():
            y = l1(x)
            assert y.dtype == tdt and torch.equal(y, ops.grouped_packed_codebook_matmul(x, c1, cen1, rows, bias=bias1, relu=True))
            z = l2(y)
            assert z.dtype == tdt and torch.equal(z, torch.tanh(ops.grouped_packed_codebook_matmul(y, c2, cen2 / 64, 32)))
    with pytest.raises(RuntimeError, match="inference only"):
        l1(torch.randn(2, kdim, device="cuda").to(tdt).requires_grad_())
    with pytest.raises(ValueError):
        compressed.GroupedPackedCompressedDense(c1, rows, cen1[:4], bias1)
    with pytest.raises(ValueError):                                      # K = 17 has no packed form
        compressed.GroupedPackedCompressedDense.from_codes(kdim, ncols, rows, lab1, torch.zeros(5, 17, device="cuda"), bias1, None)


def test_from_grouped_nbytes_and_the_state_round_trip(env):
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    kdim, ncols, k, rows = 112, 70, 16, 32
    rng = np.random.RandomState(11)
    lab, cen, bias = _layer_data(rng, kdim, ncols, k, rows)
    byte = compressed.GroupedCompressedDense(kdim, ncols, rows, lab, cen, bias, torch.relu)
    first = compressed.GroupedPackedCompressedDense.from_grouped(byte)
    assert (first.kdim, first.ncols, first.group_rows, first.bits, first.k) == (kdim, ncols, rows, 4, k)
    groups = -(-kdim // rows)
    assert first.nbytes() == kdim * packed_ref.row_bytes(ncols, 4) + 4 * groups * k + 4 * ncols == compressed.compressed_nbytes(first)
    assert first.nbytes() < byte.nbytes()
    xi = torch.from_numpy(rng.randint(-4, 5, size=(9, kdim)).astype(np.float32)).cuda()
    with torch.no_grad():
        for tdt in (torch.float32, torch.bfloat16, torch.float16):
            a, b = byte(xi.to(tdt)), first(xi.to(tdt))
            assert a.dtype == b.dtype == tdt and torch.equal(a.view(torch.int16), b.view(torch.int16)), tdt
    # the state: packed, centers, bias; loading another layer's state gives that layer's bits
    lab2, cen2, bias2 = _layer_data(rng, kdim, ncols, k, rows)
    second = compressed.GroupedPackedCompressedDense.from_codes(kdim, ncols, rows, lab2, cen2, bias2, torch.relu)
    for layer in (first, second):
        state = layer.state_dict()
        assert list(state.keys()) == ["packed", "centers", "bias"] and not list(layer.parameters())
        assert {n: t.dtype for n, t in layer.named_buffers()} == {"packed": torch.uint8, "centers": torch.float32, "bias": torch.float32}
        assert tuple(state["packed"].shape) == (ops.packed_nbytes(kdim, ncols, 4),) and tuple(state["centers"].shape) == (groups, k)
    with torch.no_grad():
        y1, y2 = first(xi), second(xi)
        assert not torch.equal(y1, y2)
        result = first.load_state_dict(second.state_dict())
        assert not result.missing_keys and not result.unexpected_keys
        assert torch.equal(first(xi).view(torch.int32), y2.view(torch.int32))


# ------------------------------------------------------------------ pack_grouped_layers on a fitted network
@pytest.fixture(scope="module")
def grouped300():
    """LeNet-300-100 with synthetic weights, pruned and quantized with group_rows = 32 (linear, 4 bits: K = 16 in every group)."""
    from neural_network_compression_amd import synth
    from neural_network_compression_amd.common import trainer as tr
    from neural_network_compression_amd.le_net_300_100_trainer import LeNet300100Trainer

    tr.Trainer.pruned_indexes_by_layer.clear()
    torch.manual_seed(0)
    t = LeNet300100Trainer()
    layers = [layer for layer in t.neural_network.get_config().values() if layer.get_weights()]
    for li, ((_, wshape, bshape), layer) in enumerate(zip(synth.LENET_300_100, layers)):
        layer.set_weights([torch.from_numpy(synth.weights(wshape, 2000 + 2 * li)).cuda(), torch.from_numpy(synth.weights(bshape, 2001 + 2 * li)).cuda()])
    x = np.random.RandomState(5).rand(64, 784).astype(np.float32)
    data = tr.LeNetDataset(x, np.zeros(64, dtype=np.int64))
    t._prune_parameters(True)
    t.quantize(data, False, 4, "linear", group_rows=32)
    return t, x


def _layerwise_within_the_float32_bound(byte_net, net, xt):
    """Layer by layer on the byte-form network's activations: a layer of ``net`` that kept its class gives the byte layer's bits, a
    packed one its result within the float32 bound of the cases, 2 kdim 2^-24 (|x| @ |W| + |bias|) (the two forms sum in different
    orders: the plans differ; the ReLU behind the product does not widen the distance)."""
    h = xt
    with torch.no_grad():
        for name in byte_net.get_config():
            a, b = getattr(byte_net, name), getattr(net, name)
            ya, yb = a(h), b(h)
            if type(a) is type(b):
                assert torch.equal(ya.view(torch.int32), yb.view(torch.int32)), name
            else:
                w = grouped_ref.weights(a.centers.cpu().numpy(), a.labels.cpu().numpy(), a.kdim, a.ncols, a.group_rows)
                mag = np.abs(h.cpu().numpy().astype(np.float64)) @ np.abs(w.astype(np.float64)) + np.abs(a.bias.cpu().numpy().astype(np.float64))
                err = np.abs(yb.cpu().numpy().astype(np.float64) - ya.cpu().numpy().astype(np.float64))
                bound = 2 * a.kdim * 2.0 ** -24 * mag
                print(f"pack_grouped_layers: {name}: largest err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.4f}")
                assert np.all(err <= bound), name
            h_last, h = h, ya
        # the networks' outputs, within the same bound at the last layer (the distance the earlier layers leave is far below it)
        last = getattr(byte_net, list(byte_net.get_config())[-1])
        w = grouped_ref.weights(last.centers.cpu().numpy(), last.labels.cpu().numpy(), last.kdim, last.ncols, last.group_rows)
        mag = np.abs(h_last.cpu().numpy().astype(np.float64)) @ np.abs(w.astype(np.float64)) + np.abs(last.bias.cpu().numpy().astype(np.float64))
        err = np.abs(net(xt).cpu().numpy().astype(np.float64) - byte_net(xt).cpu().numpy().astype(np.float64))
        bound = 2 * last.kdim * 2.0 ** -24 * mag
        print(f"pack_grouped_layers: network output: largest err / bound = {float((err / np.maximum(bound, 1e-300)).max()):.4f}")
        assert np.all(err <= bound)


def test_pack_grouped_layers(env, grouped300, tmp_path):
    from neural_network_compression_amd import compressed

    t, x = grouped300
    xt = torch.from_numpy(x).cuda()
    cnet = t.compressed_network()
    names = list(cnet.get_config())
    assert all(isinstance(layer, compressed.GroupedCompressedDense) and layer.centers.shape[1] == 16 for layer in cnet.get_config().values())
    pnet = compressed.pack_grouped_layers(cnet)                                    # packed=True: every grouped layer
    assert all(isinstance(layer, compressed.GroupedPackedCompressedDense) and layer.bits == 4 for layer in pnet.get_config().values())
    assert all(isinstance(layer, compressed.GroupedCompressedDense) for layer in cnet.get_config().values())   # a copy: cnet is as it was
    with torch.no_grad():
        got = pnet(xt)
        assert torch.equal(got.view(torch.int32), pnet(xt).view(torch.int32))      # the same bits on a second call
    _layerwise_within_the_float32_bound(cnet, pnet, xt)
    assert compressed.compressed_nbytes(pnet) < compressed.compressed_nbytes(cnet)
    for name in names:
        a, b = getattr(cnet, name), getattr(pnet, name)
        assert b.nbytes() == a.kdim * packed_ref.row_bytes(a.ncols, 4) + 4 * a.centers.numel() + 4 * a.ncols

    auto = compressed.pack_grouped_layers(cnet, packed="auto")
    kinds = {(layer.kdim, layer.ncols): type(layer) for layer in auto.get_config().values()}
    assert kinds[(100, 10)] is compressed.GroupedCompressedDense                  # rows of 16 bytes are not below rows of 10 bytes
    assert kinds[(784, 300)] is compressed.GroupedPackedCompressedDense and kinds[(300, 100)] is compressed.GroupedPackedCompressedDense
    _layerwise_within_the_float32_bound(cnet, auto, xt)

    # a grouped layer of 17 centres is left alone
    wide = compressed.pack_grouped_layers(cnet)
    last = getattr(cnet, names[-1])
    k17 = compressed.GroupedCompressedDense(last.kdim, last.ncols, 32, last.labels, torch.cat([last.centers, last.centers[:, :1]], dim=1), last.bias,
                                            last.activation)
    setattr(wide, names[-1], k17)
    again = compressed.pack_grouped_layers(wide)
    assert type(getattr(again, names[-1])) is compressed.GroupedCompressedDense and getattr(again, names[-1]).centers.shape[1] == 17
    assert type(getattr(again, names[0])) is compressed.GroupedPackedCompressedDense

    # from a stored network: the bits of packing the in-memory one
    t.store_report(str(tmp_path / "rep"))
    loaded = compressed.pack_grouped_layers(compressed.load_network(str(tmp_path / "rep" / "weights.nnc"), t.neural_network))
    for name in names:
        a, b = getattr(pnet, name), getattr(loaded, name)
        assert isinstance(b, compressed.GroupedPackedCompressedDense) and torch.equal(a.packed, b.packed), name
        assert torch.equal(a.centers.view(torch.int32), b.centers.view(torch.int32)) and torch.equal(a.bias.view(torch.int32), b.bias.view(torch.int32))
    with torch.no_grad():
        assert torch.equal(loaded(xt).view(torch.int32), got.view(torch.int32))
    for bad in (False, None, "yes", 1.5):
        with pytest.raises(ValueError, match="packed"):
            compressed.pack_grouped_layers(cnet, packed=bad)
