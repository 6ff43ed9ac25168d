"""The bitmap-sparse codebook matmul on the GPU (ops.pack_sparse_codes / sparse_codebook_matmul, csrc/nnc_cbsp.hip,
compressed.Sparse*; run with -m gpu): the packed form against a NumPy packer, exact data bit for bit against the float64 formula
in every regime the plan picks at this device, edge cases, the float32 bound on fitted weights, the layers, and the footprint."""
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_compression_amd import synth  # noqa: E402
from tests.helpers import sparse_ref  # noqa: E402
from tests.helpers.cbmm_ref import conv_nhwc, exact_grid_bits  # noqa: E402
from tests.helpers.sparse_ref import REGIME_CASES, labels_at_density, sparse_formula64  # noqa: E402

SENTINEL = 0x7FA5A5A5
Y_PAD, WS_PAD = 37, 64


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, compressed, ops, pipeline

    L = _native.load()
    _, cus = ops.device_info()
    return SimpleNamespace(L=L, ops=ops, nat=_native, compressed=compressed, pipeline=pipeline, cus=cus)


def _dev_labels(lab, lb, off=0):
    """The indices as uint8 / int16 starting ``off`` elements into a larger buffer."""
    dt = torch.uint8 if lb == 1 else torch.int16
    host = np.ascontiguousarray(lab, dtype=np.uint8 if lb == 1 else np.uint16).ravel()
    if lb == 2:
        host = host.view(np.int16)
    buf = torch.zeros(off + host.size + 8, dtype=dt, device="cuda")
    buf[off: off + host.size] = torch.from_numpy(host).cuda()
    return buf[off: off + host.size]


def _labels_host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16).astype(np.int64) if a.dtype == np.int16 else a.astype(np.int64)


def _call(env, x, m, codes, centers, bias, relu):
    """nnc_cbsp_f32 into sentinel-framed y and workspace; checks the frames; returns y (device)."""
    L = env.L
    kdim, ncols, lb = codes.kdim, codes.ncols, codes.label_bytes
    ws_bytes = int(L.nnc_cbsp_workspace_bytes(m, kdim, ncols, lb))
    mn = m * ncols
    ybuf = torch.full((mn + 2 * Y_PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    wsbuf = torch.full((ws_bytes // 4 + 2 * WS_PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    y = ybuf[Y_PAD: Y_PAD + mn]
    ws_ptr = wsbuf[WS_PAD:].data_ptr() if ws_bytes else None
    env.nat.check(L.nnc_cbsp_f32(x.data_ptr() if x is not None else None, m, kdim, codes.buf.data_ptr(), codes.nbytes(), lb, ncols,
                                 codes.zero_symbol, codes.nnz, centers.data_ptr(), centers.numel(), None if bias is None else bias.data_ptr(),
                                 int(relu), y.data_ptr(), ws_ptr, ws_bytes, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((ybuf[:Y_PAD] == SENTINEL).all()) and bool((ybuf[Y_PAD + mn:] == SENTINEL).all()), "a store outside y"
    assert bool((wsbuf[:WS_PAD] == SENTINEL).all()) and bool((wsbuf[WS_PAD + ws_bytes // 4:] == SENTINEL).all()), "a store outside the workspace"
    assert not bool((y == SENTINEL).any()), "an output left unwritten"
    return y.view(torch.float32).view(m, ncols)


def _exact_centers(rng, k, cz):
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    cen[0] = cz
    return cen


def _assert_exact(x, lab, cen, z, bias):
    """Every partial sum of the formula is a multiple of 2^-g below 2^24 grid steps: exact in float32 in any order."""
    d, cz = sparse_ref.d_table(cen, max(int(lab.max(initial=0)) + 1, cen.size), z)
    x64 = np.abs(x.astype(np.float64))
    mag = x64 @ np.where(lab != z, np.abs(d[lab]), 0.0) + abs(float(cz)) * x64.sum(axis=1, keepdims=True)
    if bias is not None:
        mag = mag + np.abs(bias)
    g = max(exact_grid_bits(x) + exact_grid_bits(d, [cz]), exact_grid_bits(bias) if bias is not None else 0)
    assert mag.max(initial=0.0) * 2.0 ** g < 2.0 ** 24


# ------------------------------------------------------------------ the form
@pytest.mark.parametrize("density", [0.0, 1e-3, 0.1, 0.5, 1.0])
@pytest.mark.parametrize("lb,k", [(1, 17), (1, 256), (2, 257), (2, 1040)])
@pytest.mark.parametrize("shape,off", [((300, 100), 0), ((37, 64), 1), ((5, 1), 3), ((129, 257), 1)])
def test_pack_matches_numpy_and_round_trips(env, density, lb, k, shape, off):
    kdim, ncols = shape
    rng = np.random.RandomState(int(density * 1000) + k + kdim)
    z = 3 % k
    lab = labels_at_density(rng, kdim, ncols, k, density, z)
    lab_t = _dev_labels(lab, lb, off)
    assert lab_t.storage_offset() == off
    codes = env.ops.pack_sparse_codes(lab_t, kdim, ncols, k, zero_symbol=z)
    ref = sparse_ref.pack_np(lab, kdim, ncols, z)
    assert codes.nnz == ref["nnz"] and codes.zero_symbol == z and codes.label_bytes == lb
    assert codes.nbytes() == env.L.nnc_cbsp_pack_bytes(kdim, ncols, lb, ref["nnz"])
    bitmap, counts, sym = sparse_ref.split_packed(codes.buf.cpu().numpy(), kdim, ncols, lb, codes.nnz)
    assert np.array_equal(bitmap, ref["bitmap"])
    assert np.array_equal(counts, ref["counts"])
    assert np.array_equal(sym.astype(np.int64), ref["symbols"])
    assert torch.equal(codes.to_dense(), lab_t)
    # the default skipped symbol is the most frequent index (ties: the lowest)
    auto = env.ops.pack_sparse_codes(lab_t, kdim, ncols, k)
    counts_all = np.bincount(lab.ravel(), minlength=k)
    assert auto.zero_symbol == int(np.argmax(counts_all))
    assert torch.equal(auto.to_dense(), lab_t)


# ------------------------------------------------------------------ exact data in every regime
def test_the_cases_hit_every_regime_at_this_device(env):
    hit = set()
    for c in REGIME_CASES:
        hit |= sparse_ref.regime_of(c, env.ops.cbsp_plan(c["m"], c["kdim"], c["ncols"], c["lb"], c["k"], env.cus))
    assert hit == sparse_ref.required_regimes(), sorted(sparse_ref.required_regimes() - hit)
    assert set(range(1, 18)) | {256, 4096} <= {c["m"] for c in REGIME_CASES}


@pytest.mark.parametrize("ci", range(len(REGIME_CASES)), ids=[sparse_ref.case_id(c) for c in REGIME_CASES])
def test_regime_case_exact(env, ci):
    """c_z = 0 and c_z != 0, with and without bias and fused ReLU: the float64 formula bit for bit; the same bits twice."""
    c = REGIME_CASES[ci]
    m, kdim, ncols, lb, k = c["m"], c["kdim"], c["ncols"], c["lb"], c["k"]
    rng = np.random.RandomState(9000 + ci)
    z = 0
    lab = labels_at_density(rng, kdim, ncols, k, c["density"], z)
    codes = env.ops.pack_sparse_codes(_dev_labels(lab, lb, c["off"]), kdim, ncols, k, zero_symbol=z)
    x = rng.randint(-8, 9, size=(m, kdim)).astype(np.float32)
    bias = rng.randint(-50, 51, size=ncols).astype(np.float32) if c["bias"] else None
    x_t = torch.from_numpy(x).cuda()
    bias_t = None if bias is None else torch.from_numpy(bias).cuda()
    for cz in (0.0, 0.75):
        cen = _exact_centers(rng, k, cz)
        _assert_exact(x, lab, cen, z, bias)
        cen_t = torch.from_numpy(cen).cuda()
        for relu in (False, True):
            y = _call(env, x_t, m, codes, cen_t, bias_t, relu)
            want = sparse_formula64(x, lab, cen, z, bias, relu).astype(np.float32)
            assert np.array_equal(y.cpu().numpy(), want), (cz, relu)
        y2 = _call(env, x_t, m, codes, cen_t, bias_t, True)
        assert torch.equal(y.view(torch.int32), y2.view(torch.int32))
        # the formula is x @ W of the decoded weights (exact data: bit for bit the dense codebook path too)
        dense = env.ops.codebook_matmul(x_t, codes.to_dense(), cen_t, kdim, ncols, bias=bias_t, relu=True)
        assert torch.equal(dense, y2), cz


# ------------------------------------------------------------------ edge cases
def test_empty_shapes(env):
    ops = env.ops
    cen = torch.tensor([0.0, 1.0, -2.0], device="cuda")
    bias = torch.tensor([1.0, -1.0, 2.0, 0.5], device="cuda")
    codes = ops.pack_sparse_codes(torch.zeros(0, dtype=torch.uint8, device="cuda"), 0, 4, 3)
    assert codes.nnz == 0 and codes.to_dense().numel() == 0
    with torch.no_grad():
        y = ops.sparse_codebook_matmul(torch.zeros(5, 0, device="cuda"), codes, cen, bias=bias, relu=True)
    assert torch.equal(y, torch.relu(bias).expand(5, 4))
    y0 = ops.sparse_codebook_matmul(torch.zeros(5, 0, device="cuda"), codes, cen)
    assert torch.equal(y0, torch.zeros(5, 4, device="cuda"))
    c2 = ops.pack_sparse_codes(torch.zeros(0, dtype=torch.uint8, device="cuda"), 7, 0, 3)
    assert ops.sparse_codebook_matmul(torch.ones(3, 7, device="cuda"), c2, cen).shape == (3, 0)
    lab = torch.tensor([0, 1, 2, 1, 0, 0], dtype=torch.uint8, device="cuda")
    c3 = ops.pack_sparse_codes(lab, 2, 3, 3)
    assert c3.zero_symbol == 0 and c3.nnz == 3
    assert ops.sparse_codebook_matmul(torch.ones(0, 2, device="cuda"), c3, cen).shape == (0, 3)
    assert ops.sparse_codebook_matmul(torch.ones(2, 4, 2, device="cuda"), c3, cen).shape == (2, 4, 3)


def test_inference_only(env):
    ops = env.ops
    codes = ops.pack_sparse_codes(torch.tensor([0, 1, 1, 0], dtype=torch.uint8, device="cuda"), 2, 2, 2)
    x = torch.ones(3, 2, device="cuda", requires_grad=True)
    cen = torch.tensor([0.0, 2.0], device="cuda")
    with pytest.raises(RuntimeError, match="inference only"):
        ops.sparse_codebook_matmul(x, codes, cen)
    with torch.no_grad():
        assert torch.equal(ops.sparse_codebook_matmul(x, codes, cen), torch.full((3, 2), 2.0, device="cuda"))


@pytest.mark.parametrize("m", [3, 40])
@pytest.mark.parametrize("lb,k,hi", [(1, 17, 256), (2, 300, 2000)])
def test_an_index_at_or_beyond_k_reads_zero(env, m, lb, k, hi):
    rng = np.random.RandomState(m + k)
    kdim, ncols = 300, 77
    lab = rng.randint(0, hi, size=(kdim, ncols))
    lab[rng.random_sample(lab.shape) < 0.6] = 5
    x = rng.randint(-8, 9, size=(m, kdim)).astype(np.float32)
    codes = env.ops.pack_sparse_codes(_dev_labels(lab, lb), kdim, ncols, k)
    assert codes.zero_symbol == 5
    for cz in (0.0, -1.25):
        cen = _exact_centers(rng, k, 0.5)
        cen[5] = cz
        cen_t = torch.from_numpy(cen).cuda()
        y = _call(env, torch.from_numpy(x).cuda(), m, codes, cen_t, None, False).cpu().numpy()
        w = np.where(lab < k, cen[np.minimum(lab, k - 1)], 0.0)
        assert np.array_equal(y, (x.astype(np.float64) @ w).astype(np.float32)), cz
        assert np.array_equal(y, sparse_formula64(x, lab, cen, 5).astype(np.float32)), cz


@pytest.mark.parametrize("m,kdim,ncols,lb,k", [(3, 20, 77, 1, 17), (5, 1200, 50, 2, 300), (16, 1100, 33, 1, 256), (40, 100, 129, 1, 17),
                                               (17, 300, 50, 2, 1040)])
def test_nonfinite_inputs_follow_the_formula(env, m, kdim, ncols, lb, k):
    """NaN / +-Inf in x and NaN in the bias against the float64 formula, with c_z = 0 (an Inf at a skipped position meets no
    weight: no NaN) and c_z != 0 (it meets c_z through the row sum); the fused ReLU keeps NaN."""
    rng = np.random.RandomState(m * 100 + kdim)
    lab = labels_at_density(rng, kdim, ncols, k, 0.3, 0)
    lab[1, :] = 0                                   # row 1 entirely skipped
    x = rng.randint(-8, 9, size=(m, kdim)).astype(np.float32)
    x[0, 1] = np.inf                                # +Inf against a skipped row
    x[1, 2] = np.nan
    x[m - 1, 5] = -np.inf
    x[m - 1, kdim - 1] = np.inf
    if m > 2:
        x[2, 7] = -np.inf
    bias = rng.randint(-50, 51, size=ncols).astype(np.float32)
    bias[4] = np.nan
    codes = env.ops.pack_sparse_codes(_dev_labels(lab, lb), kdim, ncols, k, zero_symbol=0)
    x_t, b_t = torch.from_numpy(x).cuda(), torch.from_numpy(bias).cuda()
    for cz in (0.0, 0.5):
        cen = _exact_centers(rng, k, cz)
        want = sparse_formula64(x, lab, cen, 0, bias)
        if cz == 0.0:   # row 0's +Inf sits on a skipped row of W: no NaN from it
            assert not np.isnan(np.delete(want[0], 4)).any()
        for relu in (False, True):
            y = _call(env, x_t, m, codes, torch.from_numpy(cen).cuda(), b_t, relu).cpu().numpy()
            ref = (np.where(want < 0, 0.0, want) if relu else want).astype(np.float32)
            assert np.array_equal(y, ref, equal_nan=True), (cz, relu)


def test_the_skip_rule_with_a_zero_centre(env):
    """c_z == 0: an Inf in x at a skipped position gives no NaN (the dense path gives NaN there); c_z != 0 gives Inf."""
    ops = env.ops
    lab = np.zeros((4, 3), dtype=np.int64)
    lab[2, 1] = 1
    x = np.array([[np.inf, 1.0, 2.0, 3.0]], dtype=np.float32)
    lab_t = _dev_labels(lab, 1)
    codes = ops.pack_sparse_codes(lab_t, 4, 3, 2)
    for cz, want in ((0.0, [0.0, 4.0, 0.0]), (0.5, [np.inf, np.inf, np.inf])):
        cen = torch.tensor([cz, 2.0], device="cuda")
        y = ops.sparse_codebook_matmul(torch.from_numpy(x).cuda(), codes, cen).cpu().numpy()
        assert np.array_equal(y, np.array([want], dtype=np.float32)), (cz, y)
    dense = ops.codebook_matmul(torch.from_numpy(x).cuda(), lab_t, torch.tensor([0.0, 2.0], device="cuda"), 4, 3).cpu().numpy()
    assert np.isnan(dense).all()


def test_more_than_2_pow_32_stored_symbols(env):
    """70000 x 70000 uint8 labels at 90 % density: 4.4 G stored symbols (counts past 2^31 and 2^32).  The form unpacks to the
    labels, and m = 1 (stream) and m = 17 (tiled) equal the dense codebook path on exact data."""
    ops = env.ops
    kdim = ncols = 70000
    n = kdim * ncols
    need = 3 * n + (8 << 30)
    if torch.cuda.mem_get_info()[0] < need:
        pytest.skip(f"needs {need >> 30} GiB of free device memory")
    g = torch.Generator(device="cuda").manual_seed(5)
    labels = torch.randint(0, 10, (n,), dtype=torch.uint8, device="cuda", generator=g)
    codes = ops.pack_sparse_codes(labels, kdim, ncols, 10)
    assert codes.nnz > 2 ** 32, codes
    assert int(env.L.nnc_cbsp_pack_bytes(kdim, ncols, 1, codes.nnz)) == codes.nbytes()
    back = codes.to_dense()
    assert torch.equal(back, labels)
    del back
    cen = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0, 0.25, -0.25, 0.75, -0.75, 0.125], device="cuda")
    cen[codes.zero_symbol] = 0.25
    x = torch.randint(-1, 2, (17, kdim), device="cuda", generator=g).float()
    for m in (1, 17):
        with torch.no_grad():
            ys = ops.sparse_codebook_matmul(x[:m].contiguous(), codes, cen)
            yd = ops.codebook_matmul(x[:m].contiguous(), labels, cen, kdim, ncols)
        assert torch.equal(ys, yd), m


# ------------------------------------------------------------------ fitted weights
_FITS = {}


def _fitted(env, shape, bits, mode, seed, q):
    key = (shape, bits, mode, seed, q)
    if key not in _FITS:
        w = torch.from_numpy(synth.weights(shape, seed)).cuda()
        res = env.pipeline.compress_layer(w, q=q, bits=bits, mode=mode)
        _FITS[key] = res.model
    return _FITS[key]


FITTED = [((784, 300), 4, "linear", 1), ((300, 100), 5, "density", 1), ((2450, 256), 4, "linear", 1.65), ((5000, 5000), 8, "linear", 1.65),
          ((1000, 1000), 8, "density", 1)]


@pytest.mark.parametrize("shape,bits,mode,q", FITTED)
def test_fitted_weights_within_the_float32_bound_and_deterministic(env, shape, bits, mode, q):
    ops = env.ops
    model = _fitted(env, shape, bits, mode, 5151 + shape[0], q)
    kdim, ncols = shape
    cen_np = np.ascontiguousarray(model.cluster_centers_.ravel(), dtype=np.float32)
    cen = torch.from_numpy(cen_np).cuda()
    lab_t = model.labels_compact_
    codes = ops.pack_sparse_codes(lab_t, kdim, ncols, cen.numel())
    lab = _labels_host(lab_t).reshape(kdim, ncols)
    assert codes.density() < 0.75
    rng = np.random.RandomState(kdim)
    bias = rng.standard_normal(ncols).astype(np.float32)
    for m in (1, 16, 256):
        x = rng.standard_normal((m, kdim)).astype(np.float32)
        xt = torch.from_numpy(x).cuda()
        y = ops.sparse_codebook_matmul(xt, codes, cen, bias=torch.from_numpy(bias).cuda())
        ref, bound = sparse_ref.float_bound(x, lab, cen_np, codes.zero_symbol, bias)
        err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
        assert np.all(err <= bound), (m, float((err / bound).max()))
        y2 = ops.sparse_codebook_matmul(xt, codes, cen, bias=torch.from_numpy(bias).cuda())
        assert torch.equal(y.view(torch.int32), y2.view(torch.int32))


# ------------------------------------------------------------------ footprint
def test_footprint_of_a_90_percent_pruned_layer(env):
    ops, compressed = env.ops, env.compressed
    from neural_network_compression_amd.neural_networks.layers import Dense

    rng = np.random.RandomState(90)
    kdim, ncols, k = 784, 300, 17
    lab = labels_at_density(rng, kdim, ncols, k, 0.08, 0)
    cen = torch.from_numpy(_exact_centers(rng, k, 0.0)).cuda()
    model = SimpleNamespace(cluster_centers_=cen.cpu().numpy().reshape(-1, 1), labels_compact_=_dev_labels(lab, 1))
    dense = Dense(kdim, ncols).cuda()
    dl = compressed.CompressedDense.from_dense(dense, model)
    sl = compressed.SparseCompressedDense.from_dense(dense, model)
    assert compressed.compressed_nbytes(sl) == sl.codes.nbytes() + 4 * k + 4 * ncols
    assert compressed.compressed_nbytes(sl) < 0.4 * compressed.compressed_nbytes(dl)
    assert all(t.numel() < kdim * ncols for t in sl.buffers())      # no kdim * ncols tensor resident
    # the allocator's peak while packing and multiplying a 5000 x 5000 layer: no float32 W, no per-weight int64
    kdim = ncols = 5000
    lab_t = torch.randint(0, 17, (kdim * ncols,), dtype=torch.uint8, device="cuda")
    lab_t[torch.rand(kdim * ncols, device="cuda") < 0.9] = 0
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    codes = ops.pack_sparse_codes(lab_t, kdim, ncols, 17)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    assert grown < 0.6 * kdim * ncols, grown                        # a float32 W would be 4 B / weight, an int64 8
    cen = torch.from_numpy(_exact_centers(rng, 17, 0.0)).cuda()
    for m in (1, 16, 256):
        x = torch.rand(m, kdim, device="cuda")
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = ops.sparse_codebook_matmul(x, codes, cen)
        torch.cuda.synchronize()
        # y and the split-K workspace (m x ncols partials per split) and nothing of the size of W
        ws = int(env.L.nnc_cbsp_workspace_bytes(m, kdim, ncols, 1))
        grown = torch.cuda.max_memory_allocated() - base
        assert grown <= 4 * m * ncols + ws + (2 << 20), (m, grown, ws)
        del y


# ------------------------------------------------------------------ layers
def _exact_sparse_conv(compressed, ks, cin, cout, pad, act, rng, cz, k=17):
    cen = _exact_centers(rng, k, cz)
    lab = labels_at_density(rng, ks * ks * cin, cout, k, 0.3, 0).ravel()
    bias = rng.randint(-50, 51, size=cout).astype(np.float32)
    layer = compressed.SparseCompressedConv2D.from_codes(ks, cin, cout, pad, _dev_labels(lab, 1), torch.from_numpy(cen).cuda(),
                                                         torch.from_numpy(bias).cuda(), act)
    return layer, cen[lab].reshape(ks, ks, cin, cout), bias


def _conv_ref(x, kernel, bias, pad, act):
    mag = conv_nhwc(np.abs(x), np.abs(kernel), pad) + np.abs(bias)
    g = max(exact_grid_bits(x) + exact_grid_bits(kernel), exact_grid_bits(bias))
    assert mag.max(initial=0.0) * 2.0 ** (g + 2) < 2.0 ** 24      # (+2: the formula's d = c - c_z on a grid of 1/4)
    out = conv_nhwc(x, kernel, pad) + bias
    return np.maximum(out, 0) if act is torch.relu else out


@pytest.mark.parametrize("ks", [1, 3, 5])
@pytest.mark.parametrize("padding", ["valid", "same"])
def test_sparse_conv2d_against_a_float64_convolution(env, ks, padding):
    compressed = env.compressed
    pad = ks // 2 if padding == "same" else 0
    rng = np.random.RandomState(ks * 10 + pad)
    for cin, cout, cz in ((1, 20, 0.0), (3, 16, 0.5), (20, 50, -0.25)):
        for n, (ho, wo) in ((2, (2, 3)), (3, (5, 4))):
            hh, ww = ho + ks - 1 - 2 * pad, wo + ks - 1 - 2 * pad
            act = torch.relu if cout != 16 else None
            layer, kernel, bias = _exact_sparse_conv(compressed, ks, cin, cout, pad, act, rng, cz)
            x = rng.randint(-8, 9, size=(n, hh, ww, cin)).astype(np.float32)
            with torch.no_grad():
                got = layer(torch.from_numpy(x).cuda()).cpu().numpy()
            assert got.shape == (n, ho, wo, cout)
            assert np.array_equal(got, _conv_ref(x, kernel, bias, pad, act).astype(np.float32)), (cin, cout, n)


def test_sparse_conv2d_patch_chunks_and_the_empty_batch(env, monkeypatch):
    compressed = env.compressed
    rng = np.random.RandomState(78)
    ks, cin, cout, pad = 3, 4, 16, 1
    layer, kernel, bias = _exact_sparse_conv(compressed, ks, cin, cout, pad, torch.relu, rng, 0.5)
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


def _trainer(kind):
    from neural_network_compression_amd.common import trainer as tr

    tr.Trainer.pruned_indexes_by_layer.clear()
    torch.manual_seed(0)
    if kind == "lenet300":
        from neural_network_compression_amd.le_net_300_100_trainer import LeNet300100Trainer

        t, specs = LeNet300100Trainer(), synth.LENET_300_100
    else:
        from neural_network_compression_amd.le_net_5_trainer import LeNet5Trainer

        t, specs = LeNet5Trainer(), synth.LENET_5
    layers = [layer for layer in t.neural_network.get_config().values() if layer.get_weights()]
    for li, ((_, wshape, bshape), layer) in enumerate(zip(specs, layers)):
        layer.set_weights([torch.from_numpy(synth.weights(wshape, 2000 + 2 * li)).cuda(), torch.from_numpy(synth.weights(bshape, 2001 + 2 * li)).cuda()])
    return t


def _inputs(kind, n, seed):
    rng = np.random.RandomState(seed)
    return rng.rand(n, 784).astype(np.float32) if kind == "lenet300" else rng.rand(n, 28, 28, 1).astype(np.float32)


def _sparse_layer_checks(env, t, snet, x):
    """Each sparse layer, fed what the decoded network feeds that layer, within the section 11 bound of float64 x @ W + b."""
    compressed = env.compressed
    seen = {}
    hooks = [layer.register_forward_hook(lambda mod, inp, out, name=name: seen.__setitem__(name, inp[0].detach().clone()))
             for name, layer in t.neural_network.get_config().items()]
    with torch.no_grad():
        t.neural_network(x)
    for h in hooks:
        h.remove()
    checked = 0
    for name, layer in snet.get_config().items():
        if not isinstance(layer, compressed._SparseCodebookLayer):
            continue
        inp = seen[name]
        with torch.no_grad():
            y = layer(inp).cpu().numpy()
        lab = _labels_host(layer.codes.to_dense()).reshape(layer.kdim, layer.ncols)
        cen = layer.centers.cpu().numpy()
        b = layer.bias.cpu().numpy()
        if isinstance(layer, compressed.SparseCompressedConv2D):
            p = compressed.conv_patches(inp.cpu(), layer.kernel_size, layer.pad).numpy()
            xin, y = p.reshape(-1, p.shape[-1]), y.reshape(-1, y.shape[-1])
        else:
            xin = inp.cpu().numpy()
        ref, bound = sparse_ref.float_bound(xin, lab, cen, layer.zero_symbol, b)
        if layer._fused_relu:
            ref = np.maximum(ref, 0)
        err = np.abs(y.astype(np.float64) - ref)
        assert np.all(err <= bound), (name, float((err / bound).max()))
        checked += 1
    assert checked >= 2


@pytest.mark.parametrize("kind", ["lenet300", "lenet5"])
def test_lenets_through_the_trainer(env, kind):
    from neural_network_compression_amd.common import trainer as tr

    compressed = env.compressed
    t = _trainer(kind)
    n = 512
    x = _inputs(kind, n, 7)
    t._prune_parameters(True)
    t.quantize(tr.LeNetDataset(x[:256], np.zeros(256, dtype=np.int64)), False, 4, "linear")
    xt = torch.from_numpy(x[:256]).cuda()
    snet = t.compressed_network(sparse=True)
    quantized = [name for name, l in t.neural_network.get_config().items() if t.quantized_models_by_layer.get(l, [None])[0] is not None]
    assert quantized and all(isinstance(snet.get_config()[name], compressed._SparseCodebookLayer) for name in quantized)
    _sparse_layer_checks(env, t, snet, xt)
    dnet = t.compressed_network()
    auto = t.compressed_network(sparse="auto")
    for name, layer in auto.get_config().items():   # "auto": whichever form is smaller, per layer
        if isinstance(layer, (compressed._SparseCodebookLayer, compressed._CodebookLayer)):
            other = (snet if isinstance(layer, compressed._CodebookLayer) else dnet).get_config()[name]
            assert compressed.compressed_nbytes(layer) <= compressed.compressed_nbytes(other), name
    assert compressed.compressed_nbytes(auto) <= min(compressed.compressed_nbytes(snet), compressed.compressed_nbytes(dnet))
    with torch.no_grad():
        ref, got = dnet(xt).cpu().numpy(), snet(xt).cpu().numpy()
    top2 = np.sort(ref, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 1e-4 * np.abs(ref).max()
    assert clear.sum() > 0.5 * len(ref)
    assert np.array_equal(ref.argmax(1)[clear], got.argmax(1)[clear])
    with pytest.raises(ValueError):
        t.compressed_network(sparse="yes")


def _exact_codes(net, rng, cz):
    cen = np.array([cz, 0.5, -0.5, 1.0, -1.0], dtype=np.float32)
    models = {}
    for layer in net.get_config().values():
        if not layer.get_weights():
            continue
        kl = rng.choice(5, size=layer.kernel.numel(), p=[0.86, 0.035, 0.035, 0.035, 0.035])
        bl = rng.choice(5, size=layer.bias.numel(), p=[0.4, 0.15, 0.15, 0.15, 0.15])
        kt, bt = torch.from_numpy(kl.astype(np.uint8)).cuda(), torch.from_numpy(bl.astype(np.uint8)).cuda()
        layer.set_weights([torch.from_numpy(cen[kl]).cuda().view(layer.kernel.shape), torch.from_numpy(cen[bl]).cuda()])
        models[layer] = [SimpleNamespace(cluster_centers_=cen.reshape(-1, 1), labels_compact_=kt),
                         SimpleNamespace(cluster_centers_=cen.reshape(-1, 1), labels_compact_=bt)]
    return models


@pytest.mark.parametrize("kind,cz", [("lenet300", 0.0), ("lenet300", 0.25), ("lenet5", 0.0)])
def test_lenets_bit_exact_on_exact_codebooks(env, kind, cz):
    compressed = env.compressed
    rng = np.random.RandomState(31 if kind == "lenet300" else 5)
    if kind == "lenet300":
        from neural_network_compression_amd.neural_networks.le_net_300_100 import LeNet300100

        net = LeNet300100().cuda()
        x = (rng.random_sample((64, 784)) < 0.05).astype(np.float32)
    else:
        from neural_network_compression_amd.neural_networks.le_net_5 import LeNet5

        net = LeNet5().cuda()
        x = rng.randint(0, 2, size=(3, 28, 28, 1)).astype(np.float32)
    models = _exact_codes(net, rng, cz)
    snet = compressed.compress_network(net, models, sparse=True)
    dnet = compressed.compress_network(net, models)
    assert all(isinstance(snet.get_config()[name], compressed._SparseCodebookLayer) for name, l in net.get_config().items() if l in models)
    if kind == "lenet300":   # every partial sum of the float64 forward is exact in float32
        h = x.astype(np.float64)
        for layer in net.get_config().values():
            w, b = layer.kernel.detach().cpu().numpy().astype(np.float64), layer.bias.detach().cpu().numpy().astype(np.float64)
            mag = np.abs(h) @ (np.abs(w) + abs(cz)) + np.abs(h).sum(axis=1, keepdims=True) * abs(cz) + np.abs(b)
            g = exact_grid_bits(h) + exact_grid_bits(w - cz, w)
            assert mag.max() * 2.0 ** g < 2.0 ** 24, (mag.max(), g)
            h = h @ w + b
            h = np.maximum(h, 0) if layer.activation is torch.relu else h
    xt = torch.from_numpy(x).cuda()
    with torch.no_grad():
        got, dense, dec = snet(xt), dnet(xt), net(xt)
    assert torch.equal(got.view(torch.int32), dense.view(torch.int32))
    assert torch.equal(got, dec)


@pytest.mark.parametrize("kind", ["lenet300", "lenet5"])
def test_load_network_sparse_equals_the_compressed_network(env, kind, tmp_path):
    from neural_network_compression_amd.common import trainer as tr

    compressed = env.compressed
    t = _trainer(kind)
    x = _inputs(kind, 128, 9)
    t._prune_parameters(True)
    t.quantize(tr.LeNetDataset(x, np.zeros(128, dtype=np.int64)), False, 4, "linear")
    xt = torch.from_numpy(x).cuda()
    with torch.no_grad():
        want = t.compressed_network(sparse=True)(xt)
    t.store_report(str(tmp_path / "rep"))
    loaded = compressed.load_network(str(tmp_path / "rep" / "weights.nnc"), t.neural_network, sparse=True)
    assert any(isinstance(l, compressed._SparseCodebookLayer) for l in loaded.get_config().values())
    with torch.no_grad():
        got = loaded(xt)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
