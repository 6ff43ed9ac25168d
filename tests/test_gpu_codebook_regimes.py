"""Every regime of the codebook matmul (nnc_cbmm_f32, csrc/nnc_cbmm.hip) against float64 NumPy, through the raw C ABI with
buffers the test owns (run with -m gpu).

The plan (nnc_cbmm_plan) names the regime a call takes at the device's CU count; the case list (tests/helpers/cbmm_ref.py) is
asserted to hit the whole cross product of regimes, so a plan change that orphans one fails here.  y and the workspace are slices
of larger buffers filled with a NaN sentinel no input uses: nothing outside the slices may change, nothing inside y may be left
unwritten.  Exact data (integer x, dyadic centres, integer bias) must give the float64 result bit for bit, with and without the
fused ReLU; float data stays within the float32 bound; a second call gives the same bits.  Then non-finite inputs (NaN kept
through ReLU, as torch.relu keeps it), and label / output offsets beyond 2^32 bytes and 2^31 elements."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import cbmm_ref  # noqa: E402
from tests.helpers.cbmm_ref import REGIME_CASES, matmul64, relu_like_torch  # noqa: E402

SENTINEL = 0x7FA5A5A5    # a quiet NaN whose payload neither the inputs (NumPy's NaN) nor the kernels' own NaNs carry
Y_PAD, WS_PAD = 37, 64   # sentinel words on each side of y (an odd count: y is only 4-byte aligned) and of the workspace


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, ops

    L = _native.load()
    _, cus = ops.device_info()
    assert cus >= 1
    return L, ops, cus


def _plan(ops, c, cus, addr):
    return ops.cbmm_plan(c["m"], c["kdim"], c["ncols"], c["lb"], c["k"], cus, addr)


def _dev_f32(host, view):
    """host float32 -> device; ``view``: as buf[1:] of a one-longer buffer (4-byte but not 8-byte aligned)."""
    host = np.ascontiguousarray(host, dtype=np.float32)
    if not view:
        return torch.from_numpy(host).cuda()
    buf = torch.zeros(host.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(host.ravel()).cuda()
    return buf[1:].view(host.shape)


def _dev_labels(lab, lb, off):
    """The indices as uint8 / int16 starting ``off`` elements into a buffer that has 16 spare bytes after them."""
    dt = torch.uint8 if lb == 1 else torch.int16
    host = lab.astype(np.uint8) if lb == 1 else lab.astype(np.uint16).view(np.int16)
    buf = torch.zeros(off + host.size + 16 // lb, dtype=dt, device="cuda")
    buf[off: off + host.size] = torch.from_numpy(np.ascontiguousarray(host)).cuda()
    return buf[off: off + host.size]


def _sentinel(words):
    return torch.full((words,), SENTINEL, dtype=torch.int32, device="cuda")


def _call(env, x, m, kdim, labels, lb, ncols, centers, k, bias, relu):
    """nnc_cbmm_f32 into sentinel-framed y and workspace (exactly the queried size); checks the frames; returns y (device)."""
    L, ops, _ = env
    ws_bytes = int(L.nnc_cbmm_workspace_bytes(m, kdim, ncols, lb))
    assert ws_bytes % 4 == 0
    mn = m * ncols
    ybuf, wsbuf = _sentinel(mn + 2 * Y_PAD), _sentinel(ws_bytes // 4 + 2 * WS_PAD)
    y = ybuf[Y_PAD: Y_PAD + mn]
    ws_ptr = wsbuf[WS_PAD:].data_ptr() if ws_bytes else None
    ops.nat.check(L.nnc_cbmm_f32(x.data_ptr(), m, kdim, labels.data_ptr(), lb, ncols, centers.data_ptr(), k,
                                 None if bias is None else bias.data_ptr(), int(relu), y.data_ptr(), ws_ptr, ws_bytes,
                                 torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((ybuf[:Y_PAD] == SENTINEL).all()) and bool((ybuf[Y_PAD + mn:] == SENTINEL).all()), "a store outside y"
    assert bool((wsbuf[:WS_PAD] == SENTINEL).all()) and bool((wsbuf[WS_PAD + ws_bytes // 4:] == SENTINEL).all()), "a store outside the workspace"
    assert not bool((y == SENTINEL).any()), "an output left unwritten"
    return y.view(torch.float32).view(m, ncols)


def _assert_exact_precondition(x, w, bias):
    """Integer x, quarter-integer centres, integer bias: every partial sum is a multiple of 1/4 below 2^22 / 4 in magnitude."""
    mag = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64))
    if bias is not None:
        mag = mag + np.abs(bias.astype(np.float64))
    assert 4 * mag.max(initial=0.0) < 2.0 ** 22


def _float_bound_ok(y, x, w, bias):
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    ref = x64 @ w64 + (0 if bias is None else bias.astype(np.float64))
    mag = np.abs(x64) @ np.abs(w64) + (0 if bias is None else np.abs(bias.astype(np.float64)))
    err = np.abs(y.astype(np.float64) - ref)
    bound = 2.0 * x.shape[1] * 2.0 ** -24 * mag + 1e-30
    return np.all(err <= bound), float((err / bound).max())


def test_the_cases_hit_every_regime_at_this_device(env):
    """The whole cross product: stream lb {1, 2} x mt {1, 2, 4, 8, 16} x {aligned, unaligned} x {direct, split}; tiled lb x
    {direct, split}; the uint16 table at 32 / 16 / 8 copies; 2-byte labels with K <= 256."""
    _, ops, cus = env
    hit = set()
    for c in REGIME_CASES:
        hit |= cbmm_ref.regime_of(c, _plan(ops, c, cus, 4096 + c["off"] * c["lb"]))
    assert hit == cbmm_ref.required_regimes(), sorted(cbmm_ref.required_regimes() - hit)


@pytest.mark.parametrize("ci", range(len(REGIME_CASES)), ids=[cbmm_ref.case_id(c) for c in REGIME_CASES])
def test_regime_case(env, ci):
    _, ops, cus = env
    c = REGIME_CASES[ci]
    m, kdim, ncols, lb, k = c["m"], c["kdim"], c["ncols"], c["lb"], c["k"]
    rng = np.random.RandomState(7000 + ci)
    lab = rng.randint(0, k, size=kdim * ncols)
    lab_t = _dev_labels(lab, lb, c["off"])
    # the call takes the regime the coverage test counted for it (the buffer start is 256-byte aligned)
    assert cbmm_ref.regime_of(c, _plan(ops, c, cus, lab_t.data_ptr())) == cbmm_ref.regime_of(c, _plan(ops, c, cus, 4096 + c["off"] * lb))

    # exact data: the float64 result bit for bit, with and without ReLU; the same bits a second time
    x = rng.randint(-8, 9, size=(m, kdim)).astype(np.float32)
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    bias = rng.randint(-50, 51, size=ncols).astype(np.float32) if c["bias"] else None
    w = cen[lab].reshape(kdim, ncols)
    _assert_exact_precondition(x, w, bias)
    want = x.astype(np.float64) @ w.astype(np.float64) + (0 if bias is None else bias.astype(np.float64))
    x_t, cen_t = _dev_f32(x, c["x_view"]), _dev_f32(cen, False)
    bias_t = None if bias is None else _dev_f32(bias, c["bias_view"])
    for relu in (False, True):
        y = _call(env, x_t, m, kdim, lab_t, lb, ncols, cen_t, k, bias_t, relu)
        ref = relu_like_torch(want) if relu else want
        assert np.array_equal(y.cpu().numpy(), ref.astype(np.float32)), (c, relu)
    y2 = _call(env, x_t, m, kdim, lab_t, lb, ncols, cen_t, k, bias_t, True)
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32))

    # float data: within 2 kdim 2^-24 (|x| @ |W| + |b|); deterministic
    xf = rng.standard_normal((m, kdim)).astype(np.float32)
    cf = rng.standard_normal(k).astype(np.float32)
    bf = rng.standard_normal(ncols).astype(np.float32) if c["bias"] else None
    xf_t, cf_t = _dev_f32(xf, c["x_view"]), _dev_f32(cf, False)
    bf_t = None if bf is None else _dev_f32(bf, c["bias_view"])
    y = _call(env, xf_t, m, kdim, lab_t, lb, ncols, cf_t, k, bf_t, False)
    ok, worst = _float_bound_ok(y.cpu().numpy(), xf, cf[lab].reshape(kdim, ncols), bf)
    assert ok, (c, worst)
    y2 = _call(env, xf_t, m, kdim, lab_t, lb, ncols, cf_t, k, bf_t, False)
    assert torch.equal(y.view(torch.int32), y2.view(torch.int32))


# ------------------------------------------------------------------ non-finite inputs
# (m, kdim, ncols, lb, k, path, split): the stream and tiled kernels, each direct and through the split-K combine
NONFINITE = [(3, 20, 77, 1, 17, 1, False), (5, 700, 50, 2, 300, 1, True), (16, 600, 33, 1, 256, 1, True),
             (40, 100, 129, 1, 17, 2, False), (17, 300, 50, 2, 1040, 2, True)]


@pytest.mark.parametrize("m,kdim,ncols,lb,k,path,split", NONFINITE)
def test_nonfinite_inputs_propagate_and_relu_keeps_nan(env, m, kdim, ncols, lb, k, path, split):
    """NaN and +-Inf in x, NaN in the bias; Inf against the centre that is exactly 0 gives NaN, +Inf and -Inf in one row give NaN.
    The result equals the float64 one (NaN where it is NaN), and the fused ReLU maps -Inf to 0 and keeps NaN, as torch.relu does."""
    _, ops, cus = env
    rng = np.random.RandomState(m * 1000 + kdim)
    lab = rng.randint(0, k, size=(kdim, ncols))
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    cen[0] = 0.0
    lab[2, ::3] = 0                         # row 2 meets +Inf (below) against the exact 0 centre in every third column
    x = rng.randint(-8, 9, size=(m, kdim)).astype(np.float32)
    x[0, 1] = np.nan                        # row 0: NaN
    x[1, 2] = np.inf                        # row 1: +Inf alone
    x[m - 1, 5] = -np.inf                   # row m - 1: +Inf and -Inf together
    x[m - 1, kdim - 1] = np.inf
    if m > 2:
        x[2, 7] = -np.inf                   # -Inf alone: ReLU gives 0 where the centre is positive
    bias = rng.randint(-50, 51, size=ncols).astype(np.float32)
    bias[4] = np.nan
    w = cen[lab]
    fin = np.where(np.isfinite(x), x, 0)
    _assert_exact_precondition(fin, w, np.where(np.isfinite(bias), bias, 0))
    lab_t = _dev_labels(lab.ravel(), lb, 0)
    p = ops.cbmm_plan(m, kdim, ncols, lb, k, cus, lab_t.data_ptr())
    assert p["path"] == path and (p["splits"] > 1) == split, p
    want = matmul64(x, w, bias)
    assert np.isnan(want).any() and np.isposinf(want).any() and np.isneginf(want).any()
    x_t, cen_t, bias_t = _dev_f32(x, False), _dev_f32(cen, False), _dev_f32(bias, False)
    for relu in (False, True):
        y = _call(env, x_t, m, kdim, lab_t, lb, ncols, cen_t, k, bias_t, relu).cpu().numpy()
        ref = (relu_like_torch(want) if relu else want).astype(np.float32)
        assert np.array_equal(y, ref, equal_nan=True), (relu, np.argwhere(~((y == ref) | (np.isnan(y) & np.isnan(ref))))[:5])


def test_compressed_dense_relu_keeps_nan_like_the_decoded_dense(env):
    """CompressedDense with activation=torch.relu and the decoded Dense agree on every NaN (and on every other value)."""
    from neural_network_compression_amd import compressed
    from neural_network_compression_amd.neural_networks.layers import Dense

    _, ops, _ = env
    rng = np.random.RandomState(11)
    kdim, ncols, k = 300, 100, 17
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    cen[3] = 0.0
    lab = rng.randint(0, k, size=kdim * ncols).astype(np.uint8)
    lab.reshape(kdim, ncols)[4, ::2] = 3
    bias = rng.randint(-50, 51, size=ncols).astype(np.float32)
    bias[9] = np.nan
    cen_t, lab_t = torch.from_numpy(cen).cuda(), torch.from_numpy(lab).cuda()
    dense = Dense(kdim, ncols, activation=torch.relu).cuda()
    dense.set_weights([ops.gather(cen_t, lab_t).view(kdim, ncols), torch.from_numpy(bias).cuda()])
    layer = compressed.CompressedDense(kdim, ncols, lab_t, cen_t, torch.from_numpy(bias).cuda(), torch.relu)
    assert layer._fused_relu
    for m in (1, 5, 40):
        x = rng.randint(-8, 9, size=(m, kdim)).astype(np.float32)
        x[0, 4] = np.inf
        x[m - 1, 10] = np.nan
        x[m // 2, 20] = -np.inf
        xt = torch.from_numpy(x).cuda()
        with torch.no_grad():
            got, dec = layer(xt).cpu().numpy(), dense(xt).cpu().numpy()
        ref = relu_like_torch(matmul64(x, cen[lab].reshape(kdim, ncols), bias)).astype(np.float32)
        assert np.isnan(ref).any()
        assert np.array_equal(np.isnan(got), np.isnan(dec)), m
        assert np.array_equal(got, ref, equal_nan=True), m
        assert np.array_equal(dec, ref, equal_nan=True), m


# ------------------------------------------------------------------ offsets beyond 32 / 31 bits
def _free_bytes():
    return torch.cuda.mem_get_info()[0]


def test_labels_beyond_4_gib(env):
    """kdim = ncols = 65537 uint8 indices (4.3 GB; odd ncols: unaligned rows): m = 1 (stream, split) and m = 17 (tiled)
    against a float64 product on the device, in row blocks of ops.gather-decoded indices (exact at these magnitudes)."""
    _, ops, cus = env
    kdim = ncols = 65537
    n = kdim * ncols
    assert n > 2 ** 32
    if _free_bytes() < n + (6 << 30):
        pytest.skip(f"needs {(n >> 30) + 6} GiB of free device memory")
    g = torch.Generator(device="cuda").manual_seed(3)
    labels = torch.randint(0, 5, (n,), dtype=torch.uint8, device="cuda", generator=g)
    cen = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0], device="cuda")
    x = torch.randint(-1, 2, (17, kdim), device="cuda", generator=g).float()
    bias = torch.randint(-4, 5, (ncols,), device="cuda", generator=g).float()
    p1 = ops.cbmm_plan(1, kdim, ncols, 1, 5, cus, labels.data_ptr())
    p17 = ops.cbmm_plan(17, kdim, ncols, 1, 5, cus, labels.data_ptr())
    assert p1["path"] == 1 and p1["splits"] > 1 and not p1["aligned"] and p17["path"] == 2, (p1, p17)
    t0 = time.perf_counter()
    ref = torch.zeros(17, ncols, dtype=torch.float64, device="cuda")
    mag = torch.zeros_like(ref)
    blk = 2048
    for r0 in range(0, kdim, blk):
        r1 = min(kdim, r0 + blk)
        w = ops.gather(cen, labels[r0 * ncols: r1 * ncols]).view(r1 - r0, ncols).double()
        xb = x[:, r0:r1].double()
        ref += xb @ w
        mag += xb.abs() @ w.abs()
        del w
    ref += bias.double()
    assert 4 * float((mag + bias.double().abs()).max()) < 2.0 ** 22
    t_ref = time.perf_counter() - t0
    for m in (1, 17):
        t0 = time.perf_counter()
        y = _call(env, x[:m].contiguous(), m, kdim, labels, 1, ncols, cen, 5, bias, False)
        t_call = time.perf_counter() - t0
        assert torch.equal(y, ref[:m].float()), m
        print(f"labels beyond 4 GiB: m = {m}: {t_call * 1e3:.1f} ms per checked call (reference {t_ref:.2f} s)")


def test_outputs_beyond_2_pow_31(env):
    """m * ncols > 2^31 outputs (8.6 GB) with kdim = 5 through the tiled kernel (direct), against float64 row blocks."""
    _, ops, cus = env
    m, kdim, ncols = 33000, 5, 65100
    mn = m * ncols
    assert mn > 2 ** 31
    if _free_bytes() < 4 * mn + (4 << 30):
        pytest.skip(f"needs {(4 * mn >> 30) + 4} GiB of free device memory")
    g = torch.Generator(device="cuda").manual_seed(4)
    labels = torch.randint(0, 17, (kdim * ncols,), dtype=torch.uint8, device="cuda", generator=g)
    cen = (torch.randint(-16, 17, (17,), device="cuda", generator=g) / 4.0).float()
    x = torch.randint(-8, 9, (m, kdim), device="cuda", generator=g).float()
    bias = torch.randint(-50, 51, (ncols,), device="cuda", generator=g).float()
    p = ops.cbmm_plan(m, kdim, ncols, 1, 17, cus, labels.data_ptr())
    assert p["path"] == 2 and p["splits"] == 1, p
    w = ops.gather(cen, labels).view(kdim, ncols).double()
    t0 = time.perf_counter()
    y = _call(env, x, m, kdim, labels, 1, ncols, cen, 17, bias, True)
    t_call = time.perf_counter() - t0
    blk = 2048
    for r0 in range(0, m, blk):
        xb = x[r0: r0 + blk].double()
        ref = torch.relu(xb @ w + bias.double()).float()
        assert 4 * float((xb.abs() @ w.abs() + bias.double().abs()).max()) < 2.0 ** 22
        assert torch.equal(y[r0: r0 + blk], ref), r0
    print(f"outputs beyond 2^31: {t_call * 1e3:.1f} ms per checked call")
