"""The backward pass of the bitmap-sparse codebook matmul (nnc_cbsp_dx_f32 / nnc_cbsp_dc_f32, csrc/nnc_cbspgrad.hip), the autograd
Function ops.sparse_codebook_linear, the trainable bitmap-sparse layers, compress_network_trainable and
Trainer.fine_tune_compressed(sparse=...) (run with -m gpu).

The centroid gradient must equal the dense backward's on the unpacked labels bit for bit in every regime of both plans, which the
case list is asserted to cover at the device's CU count; exact data must give the dx formula bit for bit; fitted layers stay
within the float32 bound of DESIGN.md section 13; the backward reads nothing back and allocates no kdim x ncols tensor."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_compression_amd import synth  # noqa: E402
from tests.helpers import sparse_grad_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, ops

    _native.load()
    _, cus = ops.device_info()
    return ops, cus


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_labels(lab, lb):
    host = np.ascontiguousarray(lab, dtype=np.uint8 if lb == 1 else np.uint16).ravel()
    return torch.from_numpy(host if lb == 1 else host.view(np.int16)).cuda()


def _case(ops, case, seed):
    name, m, kdim, ncols, lb, k = case[:6]
    x, g, c, lab, z = ref.case_data(case, seed)
    codes = ops.pack_sparse_codes(_dev_labels(lab, lb), kdim, ncols, k, zero_symbol=z)
    return x, g, c, lab, codes


def test_every_regime_is_covered_at_this_cu_count(env):
    ops, cus = env
    dxs = {ref.regime(ops.cbsp_dx_plan(c[1], c[2], c[3], c[4], c[5], cus)) for c in ref.REGIME_CASES}
    dcs = {ref.regime(ops.cbsp_dc_plan(c[1], c[2], c[3], c[4], c[5], cus)) for c in ref.REGIME_CASES}
    assert ref.DX_REQUIRED <= dxs and ref.DC_REQUIRED <= dcs, (ref.DX_REQUIRED - dxs, ref.DC_REQUIRED - dcs)
    assert {1, 2, 256, 257, 1040} <= {c[5] for c in ref.REGIME_CASES}
    assert {0.0, 0.01, 0.1, 0.5, 1.0} <= {c[6] for c in ref.REGIME_CASES}
    assert {1, 63, 64, 65} <= {c[3] for c in ref.REGIME_CASES} and 1 in {c[2] for c in ref.REGIME_CASES}


@pytest.mark.parametrize("case", ref.REGIME_CASES, ids=[c[0] for c in ref.REGIME_CASES])
def test_exact_data_dx_formula_and_dc_of_the_dense_backward(env, case):
    ops, cus = env
    name, m, kdim, ncols, lb, k = case[:6]
    x, g, c, lab, codes = _case(ops, case, seed=len(name) * 7 + m)
    z = codes.zero_symbol
    dxp, dcp = ops.cbsp_dx_plan(m, kdim, ncols, lb, k, cus), ops.cbsp_dc_plan(m, kdim, ncols, lb, k, cus)
    if name.startswith("stream"):       # the case hits the regime its name claims
        assert dxp["path"] == dcp["path"] == ref.PATH_STREAM
        assert ("nosplit" not in name) or dxp["splits"] == 1
        assert ("_split" not in name) or dxp["splits"] > 1
    elif name.startswith("tiled"):
        assert dxp["path"] == dcp["path"] == ref.PATH_TILED
        assert ("nosplit" not in name) or dxp["splits"] == 1
        assert ("_split" not in name) or dxp["splits"] > 1
        assert ("msplit" in name) == (dcp["splits"] > 1)
    if "zbig" in name:
        assert z >= k
    if "oob" in name:
        assert (lab[lab != z] >= k).any()
    xt, gt, ct = _cuda(x), _cuda(g), _cuda(c)
    dx = ops.sparse_codebook_matmul_dx(gt, codes, ct)
    assert dx.shape == (m, kdim) and dx.dtype == torch.float32
    assert np.array_equal(dx.cpu().numpy(), ref.dx64(g, lab, c, z)), name
    dense_labels = codes.to_dense()
    for dt in (torch.float64, torch.float32):
        dc = ops.sparse_codebook_centroid_grad(xt, gt, codes, dtype=dt)
        want = ops.codebook_centroid_grad(xt, gt, dense_labels, k, kdim, ncols, dtype=dt)
        assert dc.dtype == dt and torch.equal(dc, want), name
    # a second call gives the same bits
    assert torch.equal(ops.sparse_codebook_matmul_dx(gt, codes, ct), dx)
    assert torch.equal(ops.sparse_codebook_centroid_grad(xt, gt, codes), ops.sparse_codebook_centroid_grad(xt, gt, codes))


@pytest.mark.parametrize("m", [4, 40])
def test_dc_all_nan_and_zero_cases_match_the_dense_backward(env, m):
    ops, _ = env
    rng = np.random.RandomState(m)
    kdim, ncols, k = 70, 130, 16
    lab = ref.labels_for(rng, kdim, ncols, k, 1, 0.1, 0)
    codes = ops.pack_sparse_codes(_dev_labels(lab, 1), kdim, ncols, k, zero_symbol=0)
    x = rng.randn(m, kdim).astype(np.float32)
    g = rng.randn(m, ncols).astype(np.float32)
    i_skip = int(np.argwhere(lab[:, 0] == 0)[0, 0])
    x[1, i_skip] = np.inf                                    # an Inf in x at a skipped position
    for xx, gg in ((x, g), (np.zeros_like(x), g), (np.ones_like(x), np.zeros_like(g))):
        xt, gt = _cuda(xx), _cuda(gg)
        for dt in (torch.float64, torch.float32):
            got = ops.sparse_codebook_centroid_grad(xt, gt, codes, dtype=dt)
            want = ops.codebook_centroid_grad(xt, gt, codes.to_dense(), k, kdim, ncols, dtype=dt)
            assert torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0))
    got = ops.sparse_codebook_centroid_grad(_cuda(x), _cuda(g), codes).cpu().numpy()
    assert np.isnan(got).all()
    assert (ops.sparse_codebook_centroid_grad(_cuda(np.zeros_like(x)), _cuda(g), codes).cpu().numpy() == 0).all()


@pytest.mark.parametrize("m", [4, 40])
def test_an_inf_in_g_at_a_skipped_column_leaves_dx_finite_when_c_z_is_zero(env, m):
    ops, _ = env
    rng = np.random.RandomState(10 + m)
    kdim, ncols, k = 90, 300, 16
    lab = ref.labels_for(rng, kdim, ncols, k, 1, 0.2, 0)
    lab[:, 7] = 0                                            # column 7 fully skipped
    c = (rng.randint(-8, 9, size=k) / 4.0).astype(np.float32)
    c[0] = 0.0
    g = rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
    g[1, 7] = np.inf
    codes = ops.pack_sparse_codes(_dev_labels(lab, 1), kdim, ncols, k, zero_symbol=0)
    dx = ops.sparse_codebook_matmul_dx(_cuda(g), codes, _cuda(c)).cpu().numpy()
    assert np.isfinite(dx).all()
    g[1, 7] = 0.0
    assert np.array_equal(dx, ref.dx64(g, lab, c, 0))


def _fit(shape, seed, bits, mode, q):
    from neural_network_compression_amd import pipeline

    w = synth.weights(shape, seed)
    res = pipeline.compress_layer(torch.from_numpy(w.copy()).cuda(), q=q, bits=bits, mode=mode)
    c = res.model.cluster_centers_.ravel().astype(np.float32)
    lab = res.model.labels_.reshape(shape).astype(np.int64)
    return c, lab


@pytest.mark.parametrize("m", [1, 16, 256])
@pytest.mark.parametrize("q", [1, 1.65])
@pytest.mark.parametrize("shape,bits,mode,lb", [((784, 300), 5, "linear", 1), ((300, 100), 9, "density", 2)])
def test_fitted_layers_are_within_the_dx_bound(env, m, q, shape, bits, mode, lb):
    ops, _ = env
    c, lab = _fit(shape, 5000 + m, bits, mode, q)
    kdim, ncols = shape
    codes = ops.pack_sparse_codes(_dev_labels(lab, lb), kdim, ncols, c.size)
    rng = np.random.RandomState(m)
    x = (rng.randn(m, kdim) * 0.7).astype(np.float32)
    g = (rng.randn(m, ncols) * 1e-2).astype(np.float32)
    dx = ops.sparse_codebook_matmul_dx(_cuda(g), codes, _cuda(c)).cpu().numpy()
    want, bound = ref.dx_bound(g, lab, c, codes.zero_symbol)
    assert np.all(np.abs(dx - want) <= bound)
    dense = codes.to_dense()
    for dt in (torch.float64, torch.float32):
        assert torch.equal(ops.sparse_codebook_centroid_grad(_cuda(x), _cuda(g), codes, dtype=dt),
                           ops.codebook_centroid_grad(_cuda(x), _cuda(g), dense, c.size, kdim, ncols, dtype=dt))


# ------------------------------------------------------------------ autograd
def _layer_data(ops, m, seed, kdim=90, ncols=150, k=40, density=0.2):
    rng = np.random.RandomState(seed)
    x = (rng.randn(m, kdim) * 0.5).astype(np.float32)
    c = (rng.randn(k) * 0.1).astype(np.float32)
    lab = ref.labels_for(rng, kdim, ncols, k, 1, density, 3)
    b = (rng.randn(ncols) * 0.1).astype(np.float32)
    w = rng.randn(m, ncols).astype(np.float32)
    labels = _dev_labels(lab, 1)
    return x, c, lab, b, w, labels, ops.pack_sparse_codes(labels, kdim, ncols, k)


@pytest.mark.parametrize("m", [5, 40])
def test_sparse_codebook_linear_matches_codebook_linear(env, m):
    ops, _ = env
    x, c, lab, b, w, labels, codes = _layer_data(ops, m, m)
    grads = []
    for sparse in (True, False):
        xt, ct, bt = _cuda(x).requires_grad_(True), _cuda(c).requires_grad_(True), _cuda(b).requires_grad_(True)
        if sparse:
            y = ops.sparse_codebook_linear(xt, codes, ct, bias=bt)
        else:
            y = ops.codebook_linear(xt, labels, ct, 90, 150, bias=bt)
        (y * _cuda(w)).sum().backward()                      # linear in y: both sides receive the same g
        grads.append((xt.grad, ct.grad, bt.grad))
    (sx, sc, sb), (dx, dc, db) = grads
    assert torch.equal(sc, dc) and torch.equal(sb, db)
    want, bound = ref.dx_bound(w, lab, c, codes.zero_symbol)
    assert np.all(np.abs(sx.cpu().numpy() - want) <= bound)


@pytest.mark.parametrize("m", [5, 40])
def test_relu_masks_g_on_the_layers_own_output(env, m):
    ops, _ = env
    x, c, lab, b, w, labels, codes = _layer_data(ops, m, 100 + m)
    xt, ct = _cuda(x).requires_grad_(True), _cuda(c).requires_grad_(True)
    y = ops.sparse_codebook_linear(xt, codes, ct, bias=_cuda(b), relu=True)
    gy = _cuda(w)
    y.backward(gy)
    g = torch.where(y.detach() > 0, gy, torch.zeros((), device="cuda"))
    assert bool((y.detach() == 0).any())
    assert torch.equal(xt.grad, ops.sparse_codebook_matmul_dx(g, codes, ct.detach()))
    assert torch.equal(ct.grad, ops.sparse_codebook_centroid_grad(_cuda(x), g, codes, dtype=torch.float32))


@pytest.mark.parametrize("m", [5, 40])
def test_no_grad_forward_is_sparse_codebook_matmul(env, m):
    ops, _ = env
    x, c, lab, b, w, labels, codes = _layer_data(ops, m, 200 + m)
    xt, ct, bt = _cuda(x).requires_grad_(True), _cuda(c).requires_grad_(True), _cuda(b)
    for relu in (False, True):
        with torch.no_grad():
            assert torch.equal(ops.sparse_codebook_linear(xt, codes, ct, bias=bt, relu=relu),
                               ops.sparse_codebook_matmul(xt, codes, ct, bias=bt, relu=relu))
    with pytest.raises(RuntimeError, match="inference only"):
        ops.sparse_codebook_matmul(xt, codes, ct)


def test_forward_and_backward_read_nothing_back(env):
    ops, _ = env
    x, c, lab, b, w, labels, codes = _layer_data(ops, 16, 7)
    xt, ct, bt = _cuda(x).requires_grad_(True), _cuda(c).requires_grad_(True), _cuda(b).requires_grad_(True)
    gy = torch.ones(16, 150, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for relu in (False, True):
            ops.sparse_codebook_linear(xt, codes, ct, bias=bt, relu=relu).backward(gy)
            ops.sparse_codebook_linear(xt[:5].detach().repeat(8, 1).requires_grad_(True), codes, ct, relu=relu).backward(
                torch.ones(40, 150, device="cuda"))
    finally:
        torch.cuda.set_sync_debug_mode(0)


@pytest.mark.parametrize("m", [16, 256])
def test_backward_memory_is_outputs_plus_workspace(env, m):
    ops, cus = env
    kdim = ncols = 8192
    k = 256
    keep = torch.rand(kdim * ncols, device="cuda") < 0.1
    labels = torch.where(keep, torch.randint(1, k, (kdim * ncols,), device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda")).to(torch.uint8)
    del keep
    codes = ops.pack_sparse_codes(labels, kdim, ncols, k, zero_symbol=0)
    del labels
    ct = (torch.randn(k, device="cuda") * 0.1).requires_grad_(True)
    xt = torch.randn(m, kdim, device="cuda").requires_grad_(True)
    y = ops.sparse_codebook_linear(xt, codes, ct)
    gy = torch.randn_like(y)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y.backward(gy)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    ws = ops.cbsp_dx_plan(m, kdim, ncols, 1, k, cus)["workspace"] + ops.cbsp_dc_plan(m, kdim, ncols, 1, k, cus)["workspace"]
    outputs = m * kdim * 4 + k * 4
    assert growth <= outputs + ws + (1 << 20), (growth, outputs, ws)
    assert growth < kdim * ncols                             # no labels (64 MiB), no W (256 MiB)


# ------------------------------------------------------------------ layers
def _model(c, labels):
    from types import SimpleNamespace

    return SimpleNamespace(cluster_centers_=np.asarray(c, dtype=np.float32).reshape(-1, 1), labels_compact_=labels)


def _pruned_codes(rng, n, k, density):
    lab = ref.labels_for(rng, 1, n, k, 1, density, 0).ravel()
    c = (rng.randn(k) * 0.1).astype(np.float32)
    c[0] = 0.0
    return c, lab


@pytest.mark.parametrize("quantized_bias", [False, True])
def test_trainable_sparse_layers_match_the_inference_and_dense_trainable_ones(env, quantized_bias):
    ops, _ = env
    from neural_network_compression_amd import compressed
    from neural_network_compression_amd.neural_networks.layers import Conv2D, Dense

    rng = np.random.RandomState(31)
    torch.manual_seed(4)
    dense = Dense(784, 300, activation=torch.relu).cuda()
    conv = Conv2D(20, 50, 5, activation=torch.relu, padding="same").cuda()
    cases = ((dense, torch.randn(33, 784, device="cuda"), compressed.SparseCompressedDense, compressed.TrainableSparseCompressedDense,
              compressed.TrainableCompressedDense),
             (conv, torch.randn(3, 12, 12, 20, device="cuda"), compressed.SparseCompressedConv2D, compressed.TrainableSparseCompressedConv2D,
              compressed.TrainableCompressedConv2D))
    for layer, xin, Inf, TrSp, TrDe in cases:
        c, lab = _pruned_codes(rng, layer.kernel.numel(), 16, 0.1)
        wm = _model(c, _cuda(lab.astype(np.uint8)))
        bm = None
        if quantized_bias:
            bc, blab = _pruned_codes(rng, layer.bias.numel(), 4, 0.5)
            bm = _model(bc, _cuda(blab.astype(np.uint8)))
        make = (lambda cls: cls.from_dense(layer, wm, bm)) if isinstance(layer, Dense) else (lambda cls: cls.from_conv(layer, wm, bm))
        inf, trsp = make(Inf), make(TrSp)
        trde = compressed._trainable(layer, wm, bm)
        assert isinstance(trde, TrDe)
        with torch.no_grad():
            assert torch.equal(trsp(xin), inf(xin))
        assert torch.equal(trsp.kernel_sq_sum(), trde.kernel_sq_sum())
        assert trsp.nbytes() < trde.nbytes()
        assert compressed.compressed_nbytes(trsp) == trsp.nbytes()
        assert (trsp.bias_centers is not None) == quantized_bias
        # one backward through each: the centroid gradients agree bit for bit (no activation: both see the same g)
        trsp.activation = trde.activation = None
        trsp._fused_relu = trde._fused_relu = False
        for lay in (trsp, trde):
            (lay(xin) * 0.01).sum().backward()
        assert torch.equal(trsp.centers.grad, trde.centers.grad)


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


def _data(tr, n, seed=1):
    rng = np.random.RandomState(seed)
    x = rng.rand(n, 784).astype(np.float32)
    y = np.eye(10, dtype=np.float32)[rng.randint(0, 10, size=n)]
    return tr.LeNetDataset(x, y), tr.LeNetDataset(x[:256], y[:256].argmax(1)), x, y


def test_compress_network_trainable_dense_is_compress_network_trainable_true(env):
    from neural_network_compression_amd import compressed

    t, tr = _lenet300()
    _, test, x, _ = _data(tr, 256)
    t.quantize(test, False, 4, "linear")
    models = t.quantized_models_by_layer
    a = compressed.compress_network(t.neural_network, models, trainable=True)
    b = compressed.compress_network_trainable(t.neural_network, models, sparse=False)
    xb = torch.from_numpy(x).cuda()
    for n in ("dense1", "dense2", "out"):
        assert type(getattr(a, n)) is type(getattr(b, n)) is compressed.TrainableCompressedDense
    with torch.no_grad():
        assert torch.equal(a(xb), b(xb))
    s = compressed.compress_network_trainable(t.neural_network, models, sparse=True)
    assert all(isinstance(getattr(s, n), compressed.TrainableSparseCompressedDense) for n in ("dense1", "dense2", "out"))


def test_fine_tune_compressed_sparse_lowers_the_loss_and_keeps_the_indices(env, tmp_path):
    ops, _ = env
    from neural_network_compression_amd import compressed

    t, tr = _lenet300()
    data, test, x, y = _data(tr, 2048)
    t._prune_parameters(True)
    t.quantize(test, False, 4, "linear")
    models = t.quantized_models_by_layer
    lab0 = {(layer, ti): m.labels_compact_.clone() for layer, ms in models.items() for ti, m in enumerate(ms) if m is not None}
    c0 = {(layer, ti): m.cluster_centers_.copy() for layer, ms in models.items() for ti, m in enumerate(ms) if m is not None}
    xb, yb = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    with torch.no_grad():
        loss0 = float(t._get_error(xb, yb))
    acc = t.fine_tune_compressed(data, test, epochs=2, learning_rate=1e-3, sparse=True)
    assert len(acc) == 2 and all(0.0 <= a <= 1.0 for a in acc)
    with torch.no_grad():
        loss1 = float(t._get_error(xb, yb))
    assert loss1 < loss0, (loss0, loss1)
    moved = False
    for layer, ms in models.items():
        for ti, (w, m) in enumerate(zip(layer.get_weights(), ms)):
            if m is None:
                continue
            assert torch.equal(m.labels_compact_, lab0[(layer, ti)])
            moved |= not np.array_equal(m.cluster_centers_, c0[(layer, ti)])
            cen = torch.from_numpy(np.ascontiguousarray(m.cluster_centers_.ravel(), dtype=np.float32)).cuda()
            assert torch.equal(w.reshape(-1), ops.gather(cen, m.labels_compact_))
    assert moved
    net = t.compressed_network(trainable=True)
    t.store_compressed(str(tmp_path))
    loaded = compressed.load_network(str(tmp_path / "weights.nnc"), t.neural_network)
    with torch.no_grad():
        assert torch.equal(net(xb[:300]), loaded(xb[:300]))


def test_lenet5_fine_tunes_its_conv_layers_with_sparse_auto(env):
    from neural_network_compression_amd import compressed
    from neural_network_compression_amd import le_net_5_trainer as l5
    from neural_network_compression_amd.common import trainer as tr

    tr.Trainer.pruned_indexes_by_layer.clear()
    torch.manual_seed(3)
    t = l5.LeNet5Trainer()
    rng = np.random.RandomState(5)
    x = rng.rand(512, 28, 28, 1).astype(np.float32)
    y = np.eye(10, dtype=np.float32)[rng.randint(0, 10, size=512)]
    data, test = tr.LeNetDataset(x, y), tr.LeNetDataset(x[:128], y[:128].argmax(1))
    t.quantize(test, False, 4, "linear")
    models = t.quantized_models_by_layer
    before = {n: models[getattr(t.neural_network, n)][0].cluster_centers_.copy() for n in ("conv1", "conv2")}
    net = compressed.compress_network_trainable(t.neural_network, models, sparse="auto")
    for n in ("conv1", "conv2"):
        assert isinstance(getattr(net, n), (compressed.TrainableCompressedConv2D, compressed.TrainableSparseCompressedConv2D))
    acc = t.fine_tune_compressed(data, test, epochs=1, learning_rate=1e-2, sparse="auto")
    assert len(acc) == 1
    for n, c in before.items():
        after = models[getattr(t.neural_network, n)][0].cluster_centers_
        assert not np.array_equal(after, c), n
