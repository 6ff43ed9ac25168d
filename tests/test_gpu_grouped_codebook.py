"""The codebook matmul with one codebook per block of input rows (nnc_cbmm_grouped, csrc/nnc_cbmm_grouped.hip)
against float64 NumPy, through the raw C ABI with buffers the test owns, and through ops.grouped_codebook_matmul and
GroupedCompressedDense (run with -m gpu).

Every case of tests/helpers/grouped_ref.py with float32, bf16 and fp16 activations: exact data bit for bit (float32 output, with
and without ReLU; half output = that result rounded once), float data within the bounds of the ungrouped tests, every call into
sentinel-framed y and workspace slices and repeated for the same bits.  Then the rows on both sides of every boundary picked out
by one-hot and identity x, one group against ops.codebook_matmul bit for bit, non-finite inputs, and the layer.

The float bounds are the ungrouped ones.  float32 x (tests/test_gpu_codebook_regimes.py): 2 kdim 2^-24 (|x| @ |W| + |bias|).  Half x
(tests/test_gpu_codebook_h16.py): the products are exact, so (kdim + splits + 2) 2^-23 mag with mag = |x| @ |W_h| + |bias|, plus half
an ulp of the dtype at |ref| for a half output."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import cbmm_ref, grouped_ref, h16_ref  # noqa: E402
from tests.helpers.cbmm_ref import relu_like_torch  # noqa: E402
from tests.helpers.grouped_ref import CASES, DTYPES  # noqa: E402

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
    return grouped_ref.torch_dtype(dtype)


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


def _dev_labels(lab, off=0):
    """The indices as uint8 starting ``off`` bytes into a buffer that has 16 spare bytes after them."""
    host = np.ascontiguousarray(np.asarray(lab).ravel().astype(np.uint8))
    buf = torch.zeros(off + host.size + 16, dtype=torch.uint8, device="cuda")
    buf[off: off + host.size] = torch.from_numpy(host).cuda()
    return buf[off: off + host.size]


def _call(env, x, dtype, m, kdim, labels, ncols, centers, k, group_rows, bias, relu, half_out):
    """nnc_cbmm_grouped into sentinel-framed y and workspace (exactly the queried size); checks the frames; returns y as float32
    (device, m x ncols) and its raw bits.  A half y starts an odd number of 2-byte units into its buffer, a float32 y on a 4-byte
    boundary that is no 8-byte one."""
    L, ops, _ = env
    dt = grouped_ref.DT_CODE[dtype]
    assert not (half_out and dtype == "f32")
    ws_bytes = int(L.nnc_cbmm_grouped_workspace_bytes(dt, m, kdim, ncols))
    assert ws_bytes % 4 == 0
    mn = m * ncols
    units, pad = (mn, 37) if half_out else (2 * mn, 38)
    ybuf = torch.full((units + 2 * pad,), SENT16, dtype=torch.int16, device="cuda")
    wsbuf = torch.full((ws_bytes // 4 + 2 * WS_PAD,), SENT32, dtype=torch.int32, device="cuda")
    y = ybuf[pad: pad + units]
    ws_ptr = wsbuf[WS_PAD:].data_ptr() if ws_bytes else None
    ops.nat.check(L.nnc_cbmm_grouped(x.data_ptr(), dt, m, kdim, labels.data_ptr(), ncols, centers.data_ptr(), k, group_rows,
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


def _plan(env, c, dtype, addr):
    _, ops, cus = env
    return ops.cbmm_grouped_plan(_tdt(dtype), c["m"], c["kdim"], c["ncols"], c["k"], c["group_rows"], cus, addr)


# ------------------------------------------------------------------ the regimes at this device
def test_the_cases_hit_every_regime_at_this_device(env):
    hit, walks = set(), {}
    for c in CASES:
        for dtype in DTYPES:
            p = _plan(env, c, dtype, 4096 + c["off"])
            kernel = grouped_ref.regime_of(p, dtype)[0]
            hit.add(grouped_ref.regime_of(p, dtype))
            w = walks.setdefault(kernel, set())
            if p["max_groups_per_split"] >= 3:
                w.add("three groups in a split")
            if p["splits"] > 1 and any(lo % c["group_rows"] for lo, _ in grouped_ref.split_ranges(p, c["kdim"])):
                w.add("a split starts inside a group")
    assert hit == grouped_ref.required_regimes(), sorted(grouped_ref.required_regimes() - hit)
    for kernel in ("stream", "tiled", "mfma"):
        assert walks[kernel] == {"three groups in a split", "a split starts inside a group"}, (kernel, walks[kernel])
    _, ops, cus = env
    p = ops.cbmm_grouped_plan(torch.float32, 1, 112, 70, 3, 32, cus)
    assert (p["splits"], p["rps"]) == (3, 38), p                      # splits that start at rows 38 and 76, inside groups 1 and 2
    p = ops.cbmm_grouped_plan(torch.float32, 17, 300, 50, 256, 32, cus)
    assert (p["path"], p["splits"], p["rps"]) == (grouped_ref.PATH_TILED, 2, 150), p   # the step of rows 158..165 lies across row 160


# ------------------------------------------------------------------ every case: exact data, float data, frames, the same bits
@pytest.fixture(scope="module")
def case_data():
    """Per case, made once: labels, exact data and float data on the host (the float64 references are formed per dtype)."""
    out = []
    for ci, c in enumerate(CASES):
        lab, x, cen, bias = grouped_ref.exact_data(c, 7000 + ci)
        xf, cf, bf = grouped_ref.float_data(c, 7000 + ci)
        out.append(dict(lab=lab, x=x, cen=cen, bias=bias, xf=xf, cf=cf, bf=bf))
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[grouped_ref.case_id(c) for c in CASES])
def test_case(env, case_data, ci, dtype):
    c, d = CASES[ci], case_data[ci]
    m, kdim, ncols, k, rows = c["m"], c["kdim"], c["ncols"], c["k"], c["group_rows"]
    tdt = _tdt(dtype)
    halves = (False,) if dtype == "f32" else (False, True)
    lab_t = _dev_labels(d["lab"], c["off"])
    p = _plan(env, c, dtype, lab_t.data_ptr())
    assert grouped_ref.regime_of(p, dtype) == grouped_ref.regime_of(_plan(env, c, dtype, 4096 + c["off"]), dtype)

    # exact data: the float64 result bit for bit; the half output is that result rounded once; the same bits a second time
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
            y, bits = _call(env, x_t, dtype, m, kdim, lab_t, ncols, cen_t, k, rows, bias_t, relu, half_out)
            r = _round(ref, dtype) if half_out else ref
            got = y.cpu().numpy()
            assert np.array_equal(got, r), (c, relu, half_out, np.argwhere(got != r)[:5])
            last[half_out] = bits
    for half_out in halves:
        assert torch.equal(last[half_out], _call(env, x_t, dtype, m, kdim, lab_t, ncols, cen_t, k, rows, bias_t, True, half_out)[1])

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
        y, bits = _call(env, xf_t, dtype, m, kdim, lab_t, ncols, cf_t, k, rows, bf_t, False, half_out)
        err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
        b = bound + h16_ref.half_ulp(ref, dtype) if half_out else bound
        worst = float((err / np.maximum(b, 1e-300)).max())
        print(f"grouped float data: {grouped_ref.case_id(c)} {dtype} half_out={half_out}: largest err / bound = {worst:.4f}")
        assert np.all(err <= b), (c, dtype, half_out, worst)
        assert torch.equal(bits, _call(env, xf_t, dtype, m, kdim, lab_t, ncols, cf_t, k, rows, bf_t, False, half_out)[1])


# ------------------------------------------------------------------ the rows beside every boundary
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kdim,ncols,k,rows", [(112, 70, 16, 32), (300, 50, 256, 32), (160, 130, 3, 64)])
def test_one_hot_and_identity_x_return_the_rows_of_w(env, dtype, kdim, ncols, k, rows):
    """x = the one-hot rows that select W's rows g R - 1 and g R (m <= 16: the stream kernel, in chunks) and x = I (m = kdim: the
    tiled kernel / the MFMA tile): y is those rows of W exactly, each from its own group's table."""
    c = dict(m=1, kdim=kdim, ncols=ncols, k=k, group_rows=rows, bias=False)
    lab, _, cen, _ = grouped_ref.exact_data(c, kdim)
    w = grouped_ref.weights(cen, lab, kdim, ncols, rows, dtype)
    lab_t, cen_t = _dev_labels(lab, 1), _dev(cen, torch.float32)
    picks = sorted({r for g in range(1, -(-kdim // rows)) for r in (g * rows - 1, g * rows)} | {0, kdim - 1})
    halves = (False,) if dtype == "f32" else (False, True)
    for lo in range(0, len(picks), 6):
        sel = picks[lo: lo + 6]
        x_t = _dev(np.eye(kdim, dtype=np.float32)[sel], _tdt(dtype))
        for half_out in halves:
            y, _ = _call(env, x_t, dtype, len(sel), kdim, lab_t, ncols, cen_t, k, rows, None, False, half_out)
            assert np.array_equal(y.cpu().numpy(), w[sel]), (sel, half_out)
    x_t = _dev(np.eye(kdim, dtype=np.float32), _tdt(dtype))
    for half_out in halves:
        y, _ = _call(env, x_t, dtype, kdim, kdim, lab_t, ncols, cen_t, k, rows, None, False, half_out)
        got = y.cpu().numpy()
        assert np.array_equal(got, w), (half_out, np.argwhere(got != w)[:5])


# ------------------------------------------------------------------ one group is the ungrouped call
def _one_group_equals(env, cases, dtypes):
    _, ops, _ = env
    for ci, c in enumerate(cases):
        if c["lb"] != 1:
            continue
        m, kdim, ncols, k = c["m"], c["kdim"], c["ncols"], c["k"]
        rng = np.random.RandomState(100 + ci)
        lab_t = _dev_labels(rng.randint(0, k, size=kdim * ncols), c["off"])
        cen_t = torch.from_numpy(rng.standard_normal(k).astype(np.float32)).cuda()
        bias_t = _dev(rng.standard_normal(ncols), torch.float32, c["bias_view"]) if c["bias"] else None
        xh = rng.standard_normal((m, kdim))
        rows = -(-kdim // 32) * 32 + 32 * (ci % 3)                      # group_rows >= kdim: kdim rounded up, and beyond
        for dtype in dtypes:
            x_t = _dev(xh, _tdt(dtype), c["x_view"])
            for relu in (False, True):
                want = ops.codebook_matmul(x_t, lab_t, cen_t, kdim, ncols, bias=bias_t, relu=relu)
                got = ops.grouped_codebook_matmul(x_t, lab_t, cen_t.view(1, k), kdim, ncols, rows, bias=bias_t, relu=relu)
                assert got.dtype == want.dtype and torch.equal(got.view(torch.int16), want.view(torch.int16)), (c, dtype, relu)
            if dtype != "f32":
                want = ops.codebook_matmul(x_t, lab_t, cen_t, kdim, ncols, bias=bias_t, out_dtype=torch.float32)
                got = ops.grouped_codebook_matmul(x_t, lab_t, cen_t.view(1, k), kdim, ncols, rows, bias=bias_t, out_dtype=torch.float32)
                assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (c, dtype)


def test_one_group_equals_codebook_matmul_float32(env):
    """group_rows >= kdim on the uint8 cases of cbmm_ref.REGIME_CASES, float data: ops.codebook_matmul's bits."""
    _one_group_equals(env, cbmm_ref.REGIME_CASES, ("f32",))


def test_one_group_equals_codebook_matmul_half(env):
    """The same on the uint8 cases of h16_ref.CASES in bf16 and fp16, half and float32 output."""
    _one_group_equals(env, h16_ref.CASES, ("bf16", "fp16"))


# ------------------------------------------------------------------ non-finite inputs, indices >= K
# (m, kdim, ncols, k, path for float32 x, path for half x, split): every kernel, direct and through the split-K combine
NONFINITE = [(4, 112, 77, 16, 1, 1, False), (3, 112, 70, 3, 1, 1, True), (17, 112, 130, 16, 2, 5, False), (17, 300, 50, 17, 2, 5, True)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,kdim,ncols,k,path32,path16,split", NONFINITE)
def test_nonfinite_inputs_propagate_and_an_index_past_k_reads_zero(env, dtype, m, kdim, ncols, k, path32, path16, split):
    """NaN and +-Inf in x, NaN in the bias; Inf against a centre that is exactly 0 gives NaN; an index >= K reads 0 in every group
    (and Inf against it NaN).  The result equals the float64 one (NaN where it is NaN); the fused ReLU maps -Inf to 0 and keeps NaN."""
    _, ops, cus = env
    rows = 32
    c = dict(m=m, kdim=kdim, ncols=ncols, k=k, group_rows=rows, bias=True)
    lab, x, cen, bias = grouped_ref.exact_data(c, m * 1000 + kdim)
    lab = lab.reshape(kdim, ncols)
    cen[:, 0] = 0.0
    lab[34, ::3] = 0                        # row 34 (group 1) meets +Inf against the exact 0 centre in every third column,
    lab[34, 1::3] = 255                     # against an index >= K in the next ones;
    lab[9, :] = min(255, k + 3)             # rows of indices >= K in groups 0 and 2
    lab[70, :] = k
    x[0, 1] = np.nan
    x[1, 34] = np.inf                       # +Inf where W[34] > 0, NaN against the 0 centre and the index >= K
    x[2, 64] = -np.inf                      # group 2's centres are positive: -Inf
    if m > 3:
        x[m - 1, kdim - 1] = np.inf
        x[m - 1, 5] = -np.inf
    bias[4] = np.nan
    w = grouped_ref.weights(cen, lab, kdim, ncols, rows, dtype)
    assert k == 256 or np.all(w[9] == 0)
    cbmm_ref.assert_exact(np.where(np.isfinite(x), x, 0), w, np.where(np.isfinite(bias), bias, 0))
    lab_t = _dev_labels(lab)
    p = ops.cbmm_grouped_plan(_tdt(dtype), m, kdim, ncols, k, rows, cus, lab_t.data_ptr())
    assert p["path"] == (path32 if dtype == "f32" else path16) and (p["splits"] > 1) == split, p
    want = grouped_ref.reference(x, w, bias)
    assert np.isnan(want).any() and np.isposinf(want).any() and np.isneginf(want).any()
    x_t, cen_t, bias_t = _dev(x, _tdt(dtype)), _dev(cen, torch.float32), _dev(bias, torch.float32)
    for relu in (False, True):
        ref = (relu_like_torch(want) if relu else want).astype(np.float32)
        for half_out in ((False,) if dtype == "f32" else (False, True)):
            y = _call(env, x_t, dtype, m, kdim, lab_t, ncols, cen_t, k, rows, bias_t, relu, half_out)[0].cpu().numpy()
            r = _round(ref, dtype) if half_out else ref
            assert np.array_equal(y, r, equal_nan=True), (relu, half_out, np.argwhere(~((y == r) | (np.isnan(y) & np.isnan(r))))[:5])


def test_degenerate_shapes(env):
    """m = 0 and ncols = 0 write nothing; kdim = 0 writes the bias (ReLU applied), in float32 and in half."""
    _, ops, _ = env
    cen_t = torch.ones(1, 4, device="cuda")
    lab_t = torch.zeros(16, dtype=torch.uint8, device="cuda")
    bias = np.array([-1.5, 2.25, 0.0, 1000.0, -3.0], dtype=np.float32)
    bias_t = torch.from_numpy(bias).cuda()
    for dtype in DTYPES:
        x_t = torch.zeros(8, dtype=_tdt(dtype), device="cuda")
        for half_out in ((False,) if dtype == "f32" else (False, True)):
            y, _ = _call(env, x_t, dtype, 3, 0, lab_t, 5, cen_t, 4, 32, bias_t, True, half_out)
            assert np.array_equal(y.cpu().numpy(), np.tile(np.maximum(bias, 0), (3, 1)))
        x2 = torch.zeros((0, 40), dtype=_tdt(dtype), device="cuda")
        cen2 = torch.ones(2, 4, device="cuda")
        assert ops.grouped_codebook_matmul(x2, torch.zeros(40 * 5, dtype=torch.uint8, device="cuda"), cen2, 40, 5, 32).shape == (0, 5)
        assert ops.grouped_codebook_matmul(x_t.view(1, 8), torch.zeros(0, dtype=torch.uint8, device="cuda"), cen_t, 8, 0, 32).shape == (1, 0)


# ------------------------------------------------------------------ ops and the layer
def _layer_data(rng, kdim, ncols, k, rows):
    c = dict(m=1, kdim=kdim, ncols=ncols, k=k, group_rows=rows, bias=True)
    lab, _, cen, bias = grouped_ref.exact_data(c, rng.randint(1 << 20))
    return torch.from_numpy(lab.astype(np.uint8)).cuda(), torch.from_numpy(cen).cuda(), torch.from_numpy(bias).cuda()


def test_ops_argument_and_dtype_rules(env):
    _, ops, _ = env
    kdim, ncols, k, rows = 112, 70, 16, 32
    lab_t, cen_t, bias_t = _layer_data(np.random.RandomState(1), kdim, ncols, k, rows)
    x = torch.from_numpy(np.random.RandomState(2).randint(-4, 5, size=(2, 5, kdim)).astype(np.float32)).cuda()
    y32 = ops.grouped_codebook_matmul(x, lab_t, cen_t, kdim, ncols, rows, bias=bias_t)
    assert y32.shape == (2, 5, ncols) and y32.dtype == torch.float32
    w = grouped_ref.weights(cen_t.cpu().numpy(), lab_t.cpu().numpy(), kdim, ncols, rows)
    assert np.array_equal(y32.cpu().numpy().reshape(10, ncols), (grouped_ref.reference(x.cpu().numpy().reshape(10, kdim), w, bias_t.cpu().numpy())).astype(np.float32))
    for tdt in (torch.bfloat16, torch.float16):
        yf = ops.grouped_codebook_matmul(x.to(tdt), lab_t, cen_t, kdim, ncols, rows, bias=bias_t, out_dtype=torch.float32)
        yh = ops.grouped_codebook_matmul(x.to(tdt), lab_t, cen_t, kdim, ncols, rows, bias=bias_t)
        assert yf.dtype == torch.float32 and yh.dtype == tdt and torch.equal(yh, yf.to(tdt))
        with pytest.raises(TypeError):
            ops.grouped_codebook_matmul(x.to(tdt), lab_t, cen_t, kdim, ncols, rows, out_dtype=torch.float64)
        with pytest.raises(TypeError):
            ops.grouped_codebook_matmul(x.to(tdt), lab_t, cen_t.to(tdt), kdim, ncols, rows)
        with pytest.raises(RuntimeError, match="inference only"):
            ops.grouped_codebook_matmul(x.to(tdt).requires_grad_(), lab_t, cen_t, kdim, ncols, rows)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.grouped_codebook_matmul(x.clone().requires_grad_(), lab_t, cen_t, kdim, ncols, rows)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.grouped_codebook_matmul(x, lab_t, cen_t.clone().requires_grad_(), kdim, ncols, rows)
    with torch.no_grad():
        assert torch.equal(ops.grouped_codebook_matmul(x.clone().requires_grad_(), lab_t, cen_t, kdim, ncols, rows, bias=bias_t), y32)
    with pytest.raises(TypeError):
        ops.grouped_codebook_matmul(x.double(), lab_t, cen_t, kdim, ncols, rows)
    with pytest.raises(TypeError, match="uint8"):                        # two-byte labels: there is no such form
        ops.grouped_codebook_matmul(x, lab_t.to(torch.int16), cen_t, kdim, ncols, rows)
    for bad_rows in (0, 16, 48, -32):
        with pytest.raises(ValueError, match="group_rows"):
            ops.grouped_codebook_matmul(x, lab_t, cen_t, kdim, ncols, bad_rows)
    with pytest.raises(ValueError, match="centers"):                     # 4 groups need 4 codebooks
        ops.grouped_codebook_matmul(x, lab_t, cen_t[:3].contiguous(), kdim, ncols, rows)
    with pytest.raises(ValueError, match="centers"):
        ops.grouped_codebook_matmul(x, lab_t, cen_t.reshape(-1), kdim, ncols, rows)
    with pytest.raises(ValueError, match="centers"):                     # K > 256
        ops.grouped_codebook_matmul(x, lab_t, torch.zeros(4, 257, device="cuda"), kdim, ncols, rows)


@pytest.mark.parametrize("tdt", [torch.float32, torch.bfloat16, torch.float16])
def test_layer_matches_the_op_and_a_chain_stays_in_its_dtype(env, tdt):
    from neural_network_compression_amd import compressed

    _, ops, _ = env
    kdim, ncols, k, rows = 300, 100, 16, 64
    rng = np.random.RandomState(3)
    lab1, cen1, bias1 = _layer_data(rng, kdim, ncols, k, rows)
    lab2, cen2, _ = _layer_data(rng, ncols, kdim, k, 32)
    l1 = compressed.GroupedCompressedDense.from_codes(kdim, ncols, rows, lab1, cen1, bias1, torch.relu)
    l2 = compressed.GroupedCompressedDense(ncols, kdim, 32, lab2, cen2 / 64, None, torch.tanh)
    assert l1.nbytes() == kdim * ncols + 5 * k * 4 + ncols * 4 == compressed.compressed_nbytes(l1)
    assert l1.get_weights() == []
    for m in (1, 5, 40):
        x = torch.randn(m, kdim, device="cuda").to(tdt)
        with torch.no_grad():
            y = l1(x)
            assert y.dtype == tdt and torch.equal(y, ops.grouped_codebook_matmul(x, lab1, cen1, kdim, ncols, rows, bias=bias1, relu=True))
            z = l2(y)
            assert z.dtype == tdt and torch.equal(z, torch.tanh(ops.grouped_codebook_matmul(y, lab2, cen2 / 64, ncols, kdim, 32)))
    with pytest.raises(RuntimeError, match="inference only"):
        l1(torch.randn(2, kdim, device="cuda").to(tdt).requires_grad_())
    with pytest.raises(ValueError):
        compressed.GroupedCompressedDense(kdim, ncols, rows, lab1, cen1[:4], bias1)
    with pytest.raises(TypeError):
        compressed.GroupedCompressedDense(kdim, ncols, rows, lab1.to(torch.int16), cen1, bias1)
