"""The backward pass of the codebook matmul (nnc_cbmm_dx_f32 / nnc_cbmm_dc_f32, csrc/nnc_cbgrad.hip), the autograd Function
ops.codebook_linear, the trainable compressed layers and Trainer.fine_tune_compressed (run with -m gpu).

Exact data (integer x and g, dyadic centres) must give the float64 formulas bit for bit in every regime of both plans, which the
case list is asserted to cover at the device's CU count.  Fitted data stays within the float32 bounds of DESIGN.md section 12;
the same call gives the same bits; the backward allocates no W-sized buffer and reads nothing back to the host."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_compression_amd import synth  # noqa: E402
from tests.helpers import cbgrad_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, ops

    _native.load()
    _, cus = ops.device_info()
    return ops, cus


def _dev_labels(lab, lb, off):
    """The indices as uint8 / int16 starting ``off`` elements into a buffer with 16 spare bytes after them."""
    dt = torch.uint8 if lb == 1 else torch.int16
    host = lab.astype(np.uint8) if lb == 1 else lab.astype(np.uint16).view(np.int16)
    buf = torch.zeros(off + host.size + 16 // lb, dtype=dt, device="cuda")
    buf[off: off + host.size] = torch.from_numpy(np.ascontiguousarray(host).ravel()).cuda()
    return buf[off: off + host.size]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_every_regime_is_covered_at_this_cu_count(env):
    ops, cus = env
    dxs, dcs = set(), set()
    for case in ref.REGIME_CASES:
        _, m, kdim, ncols, lb, k, off, _ = case
        lab = _dev_labels(np.zeros((kdim, ncols), dtype=np.int64), lb, off)
        dxs.add(ref.dx_regime(ops.cbmm_dx_plan(m, kdim, ncols, lb, k, cus, lab.data_ptr())))
        dcs.add(ref.dc_regime(ops.cbmm_dc_plan(m, kdim, ncols, lb, k, cus, lab.data_ptr())))
    assert ref.DX_REQUIRED <= dxs and ref.DC_REQUIRED <= dcs, (ref.DX_REQUIRED - dxs, ref.DC_REQUIRED - dcs)


@pytest.mark.parametrize("case", ref.REGIME_CASES, ids=[c[0] for c in ref.REGIME_CASES])
def test_exact_data_matches_float64_bit_for_bit(env, case):
    ops, cus = env
    name, m, kdim, ncols, lb, k, off, _ = case
    x, g, c, lab = ref.case_data(case, seed=len(name) * 7 + m)
    labels = _dev_labels(lab, lb, off)
    dxp = ops.cbmm_dx_plan(m, kdim, ncols, lb, k, cus, labels.data_ptr())
    dcp = ops.cbmm_dc_plan(m, kdim, ncols, lb, k, cus, labels.data_ptr())
    # the case hits the regime its name claims
    if name.startswith("stream"):
        assert dxp["path"] == dcp["path"] == ref.PATH_STREAM
        assert ("nosplit" not in name) or dxp["splits"] == 1
        assert ("_split" not in name) or dxp["splits"] > 1
        assert ("aligned" not in name or "unaligned" in name) or dxp["aligned"] == dcp["aligned"] == 1
        assert ("unaligned" not in name) or dxp["aligned"] == dcp["aligned"] == 0
    elif name.startswith("tiled"):
        assert dxp["path"] == dcp["path"] == ref.PATH_TILED
        assert ("_split" not in name) or dxp["splits"] > 1
        assert ("msplit" in name) == (dcp["splits"] > 1)
    gt, xt, ct = _cuda(g), _cuda(x), _cuda(c)
    dx = ops.codebook_matmul_dx(gt, labels, ct, kdim, ncols)
    dc = ops.codebook_centroid_grad(xt, gt, labels, k, kdim, ncols)
    dc32 = ops.codebook_centroid_grad(xt, gt, labels, k, kdim, ncols, dtype=torch.float32)
    assert dx.shape == (m, kdim) and dx.dtype == torch.float32 and dc.shape == (k,) and dc.dtype == torch.float64
    want_dx = ref.dx64(g, lab, c)
    want_dc = ref.dc64(x, g, lab, k) if m * kdim * ncols else np.zeros(k)
    assert np.array_equal(dx.cpu().numpy(), want_dx), name
    assert np.array_equal(dc.cpu().numpy(), want_dc), name
    assert np.array_equal(dc32.cpu().numpy(), want_dc.astype(np.float32)), name
    # a second call gives the same bits
    assert torch.equal(ops.codebook_matmul_dx(gt, labels, ct, kdim, ncols), dx)
    assert torch.equal(ops.codebook_centroid_grad(xt, gt, labels, k, kdim, ncols), dc)


def test_non_finite_inputs(env):
    ops, _ = env
    case = ("nf", 4, 70, 130, 1, 16, 0, False)
    x, g, c, lab = ref.case_data(case, 3)
    labels = _dev_labels(lab, 1, 0)
    x[1, 5] = np.inf
    dc = ops.codebook_centroid_grad(_cuda(x), _cuda(g), labels, 16, 70, 130).cpu().numpy()
    assert np.isnan(dc).all()
    c[lab[0, 0]] = np.nan                                     # dx: a NaN centre reaches exactly the rows whose indices select it
    dx = ops.codebook_matmul_dx(_cuda(g), labels, _cuda(c), 70, 130).cpu().numpy()
    with np.errstate(invalid="ignore"):
        want = ref.dx64(g, lab, c)
    assert np.array_equal(np.isnan(dx), np.isnan(want))


def _fit(ops, shape, seed, bits, mode, lb):
    from neural_network_compression_amd import pipeline

    w = synth.weights(shape, seed)
    res = pipeline.compress_layer(torch.from_numpy(w.copy()).cuda(), q=1, bits=bits, mode=mode)
    c = res.model.cluster_centers_.ravel().astype(np.float32)
    lab = res.model.labels_.reshape(shape).astype(np.int64)
    return c, lab, _dev_labels(lab, lb, 0)


@pytest.mark.parametrize("m", [1, 7, 16, 64, 300])
@pytest.mark.parametrize("shape,bits,mode,lb", [((784, 300), 5, "linear", 1), ((300, 100), 9, "density", 2), ((2450, 256), 8, "density", 2)])
def test_fitted_data_is_within_the_float32_bounds(env, m, shape, bits, mode, lb):
    ops, cus = env
    c, lab, labels = _fit(ops, shape, 4000 + m, bits, mode, lb)
    k = c.size
    kdim, ncols = shape
    rng = np.random.RandomState(m)
    x = (rng.randn(m, kdim) * 0.7).astype(np.float32)
    g = (rng.randn(m, ncols) * 1e-2).astype(np.float32)
    dx = ops.codebook_matmul_dx(_cuda(g), labels, _cuda(c), kdim, ncols).cpu().numpy()
    assert np.all(np.abs(dx - ref.dx64(g, lab, c)) <= ref.dx_bound(g, lab, c))
    t = ops.cbmm_dc_plan(m, kdim, ncols, lb, k, cus)["terms_log2"]
    S, flag = ops.cbgrad_shift(m, np.abs(x).max(), np.abs(g).max(), t)
    assert flag == ops.CBGRAD_OK
    for dt, f32 in ((torch.float64, False), (torch.float32, True)):
        dc = ops.codebook_centroid_grad(_cuda(x), _cuda(g), labels, k, kdim, ncols, dtype=dt).cpu().numpy().astype(np.float64)
        assert np.all(np.abs(dc - ref.dc64(x, g, lab, k)) <= ref.dc_bound(x, g, lab, k, S, f32_out=f32))
    again = ops.codebook_centroid_grad(_cuda(x), _cuda(g), labels, k, kdim, ncols).cpu().numpy()
    assert np.array_equal(again, ops.codebook_centroid_grad(_cuda(x), _cuda(g), labels, k, kdim, ncols).cpu().numpy())


# ------------------------------------------------------------------ autograd
def _exact_layer(m=6, kdim=90, ncols=150, k=40, seed=0):
    rng = np.random.RandomState(seed)
    x = rng.randint(-3, 4, size=(m, kdim)).astype(np.float32)
    c = (rng.randint(-8, 9, size=k) / 4.0).astype(np.float32)
    lab = rng.randint(0, k, size=(kdim, ncols))
    b = rng.randint(-5, 6, size=ncols).astype(np.float32)
    return x, c, lab, b


@pytest.mark.parametrize("m", [5, 40])
def test_codebook_linear_no_grad_equals_codebook_matmul(env, m):
    ops, _ = env
    x, c, lab, b = _exact_layer(m=m)
    xt = (_cuda(x) * 0.37).requires_grad_(True)
    ct, bt, labels = _cuda(c).requires_grad_(True), _cuda(b).requires_grad_(True), _dev_labels(lab, 1, 1)
    for relu in (False, True):
        with torch.no_grad():
            y = ops.codebook_linear(xt, labels, ct, 90, 150, bias=bt, relu=relu)
            want = ops.codebook_matmul(xt, labels, ct, 90, 150, bias=bt, relu=relu)
        assert torch.equal(y, want)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.codebook_matmul(xt, labels, ct, 90, 150)


@pytest.mark.parametrize("m", [5, 40])
@pytest.mark.parametrize("relu", [False, True])
def test_codebook_linear_gradients_match_the_exact_formulas(env, m, relu):
    ops, _ = env
    x, c, lab, b = _exact_layer(m=m, seed=m)
    rng = np.random.RandomState(m + 1)
    gy = rng.randint(-3, 4, size=(m, 150)).astype(np.float32)
    xt, ct, bt = _cuda(x).requires_grad_(True), _cuda(c).requires_grad_(True), _cuda(b).requires_grad_(True)
    labels = _dev_labels(lab, 1, 0)
    y = ops.codebook_linear(xt, labels, ct, 90, 150, bias=bt, relu=relu)
    y.backward(_cuda(gy))
    y64 = x.astype(np.float64) @ ref.decoded(lab, c) + b
    g = np.where(y64 > 0, gy, 0.0) if relu else gy.astype(np.float64)
    assert np.array_equal(y.detach().cpu().numpy(), np.maximum(y64, 0) if relu else y64)
    assert np.array_equal(xt.grad.cpu().numpy(), ref.dx64(g, lab, c))
    assert np.array_equal(ct.grad.cpu().numpy(), ref.dc64(x, g, lab, 40).astype(np.float32))
    assert np.array_equal(bt.grad.cpu().numpy(), g.sum(0))


def test_relu_gives_nan_and_negative_outputs_a_zero_gradient(env):
    ops, _ = env
    x, c, lab, b = _exact_layer(m=4, seed=9)
    x[0, 3] = np.nan                                          # row 0 of y is NaN
    xt, ct = _cuda(x).requires_grad_(True), _cuda(c)
    labels = _dev_labels(lab, 1, 0)
    y = ops.codebook_linear(xt, labels, ct, 90, 150, relu=True)
    yh = y.detach().cpu().numpy()
    assert np.isnan(yh[0]).all() and (yh[1:] == 0).any()
    y.backward(torch.ones_like(y))
    mask = np.where(np.nan_to_num(yh, nan=-1.0) > 0, 1.0, 0.0)
    got = xt.grad.cpu().numpy()
    assert (got[0] == 0).all()
    assert np.array_equal(got, ref.dx64(mask, lab, c))


def test_only_the_needed_kernels_run(env, monkeypatch):
    ops, _ = env
    x, c, lab, b = _exact_layer(m=3)
    labels = _dev_labels(lab, 1, 0)
    calls = []
    real_dx, real_dc = ops.codebook_matmul_dx, ops.codebook_centroid_grad
    monkeypatch.setattr(ops, "codebook_matmul_dx", lambda *a, **k: calls.append("dx") or real_dx(*a, **k))
    monkeypatch.setattr(ops, "codebook_centroid_grad", lambda *a, **k: calls.append("dc") or real_dc(*a, **k))
    ops.codebook_linear(_cuda(x).requires_grad_(True), labels, _cuda(c), 90, 150).sum().backward()
    assert calls == ["dx"]
    calls.clear()
    ops.codebook_linear(_cuda(x), labels, _cuda(c).requires_grad_(True), 90, 150).sum().backward()
    assert calls == ["dc"]


def test_forward_and_backward_read_nothing_back(env):
    ops, _ = env
    x, c, lab, b = _exact_layer(m=16)
    xt, ct, bt = _cuda(x).requires_grad_(True), _cuda(c).requires_grad_(True), _cuda(b).requires_grad_(True)
    labels = _dev_labels(lab, 1, 0)
    gy = torch.ones(16, 150, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for relu in (False, True):
            ops.codebook_linear(xt, labels, ct, 90, 150, bias=bt, relu=relu).backward(gy)
            ops.codebook_linear(xt[:5].detach().repeat(8, 1).requires_grad_(True), labels, ct, 90, 150, relu=relu).backward(
                torch.ones(40, 150, device="cuda"))
    finally:
        torch.cuda.set_sync_debug_mode(0)


@pytest.mark.parametrize("m", [16, 256])
def test_backward_memory_is_outputs_plus_workspace(env, m):
    ops, cus = env
    kdim = ncols = 8192
    k = 256
    labels = torch.randint(0, k, (kdim * ncols,), dtype=torch.uint8, device="cuda")
    ct = (torch.randn(k, device="cuda") * 0.1).requires_grad_(True)
    xt = torch.randn(m, kdim, device="cuda").requires_grad_(True)
    y = ops.codebook_linear(xt, labels, ct, kdim, ncols)
    gy = torch.randn_like(y)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y.backward(gy)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    ws = ops.cbmm_dx_plan(m, kdim, ncols, 1, k, cus)["workspace"] + ops.cbmm_dc_plan(m, kdim, ncols, 1, k, cus)["workspace"]
    outputs = m * kdim * 4 + k * 4
    assert growth <= outputs + ws + (1 << 20), (growth, outputs, ws)
    assert growth < kdim * ncols * 4 // 4


# ------------------------------------------------------------------ trainable layers
@pytest.mark.parametrize("padding", ["same", "valid"])
def test_trainable_conv_gradients_match_the_float_layer(env, padding):
    ops, _ = env
    from neural_network_compression_amd import compressed
    from neural_network_compression_amd.neural_networks.layers import Conv2D

    torch.manual_seed(1)
    conv = Conv2D(3, 8, 5, activation=torch.relu, padding=padding).cuda()
    k = 12
    rng = np.random.RandomState(2)
    c = (rng.randn(k) * 0.2).astype(np.float32)
    lab = rng.randint(0, k, size=conv.kernel.numel())
    ct = _cuda(c)
    lab_t = _cuda(lab.astype(np.uint8))
    conv.set_weights([ops.gather(ct, lab_t).view(conv.kernel.shape), torch.full((8,), 0.05, device="cuda")])
    layer = compressed.TrainableCompressedConv2D(5, 3, 8, conv.pad, compressed._unfold_labels(5, 3, 8, lab_t), ct, conv.bias.detach(),
                                                 None, torch.relu)
    x = torch.randn(3, 11, 11, 3, device="cuda")
    gy_shape = conv(x).shape
    gy = torch.randn(gy_shape, device="cuda")
    xa = x.clone().requires_grad_(True)
    layer(xa).backward(gy)
    # float64 reference on the decoded kernel
    conv64 = copy.deepcopy(conv).double().cpu()
    x64 = x.double().cpu().requires_grad_(True)
    y64 = conv64(x64)
    y64.backward(gy.double().cpu())
    dc64 = np.bincount(lab, weights=conv64.kernel.grad.numpy().ravel(), minlength=k)
    # magnitudes for the bound: |x| and |g| through the same float64 path
    conva = copy.deepcopy(conv64)
    conva.set_weights([conv64.kernel.detach().abs(), torch.zeros(8, dtype=torch.float64)])
    conva.activation = None
    xa64 = x64.detach().abs().requires_grad_(True)
    mask = (y64 > 0).double()
    conva(xa64).backward((gy.double().cpu() * mask).abs())
    n_o, n_i = 8 * 25, xa.shape[0] * gy_shape[1] * gy_shape[2]
    bx = 2.0 * (n_o + 4) * ref.U * xa64.grad.numpy() + 1e-30
    assert np.all(np.abs(xa.grad.double().cpu().numpy() - x64.grad.numpy()) <= bx)
    mag = np.bincount(lab, weights=conva.kernel.grad.numpy().ravel(), minlength=k)
    bc = 2.0 * (n_i + 4) * ref.U * mag + ref.U * np.abs(dc64) + 2.0 ** -40
    assert np.all(np.abs(layer.centers.grad.double().cpu().numpy() - dc64) <= bc)


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


def test_one_batch_of_fine_tune_compressed_is_the_float64_step(env):
    t, tr = _lenet300()
    data, test, x, y = _data(tr, 512)
    t.quantize(test, False, 4, "linear")
    models = t.quantized_models_by_layer
    c0 = {(layer, ti): m.cluster_centers_.ravel().copy() for layer, ms in models.items() for ti, m in enumerate(ms) if m is not None}
    labels = {(layer, ti): m.labels_compact_.cpu().numpy().astype(np.int64).ravel() for layer, ms in models.items() for ti, m in enumerate(ms) if m is not None}
    net64 = copy.deepcopy(t.neural_network).double().cpu()
    loss = t._get_error(torch.from_numpy(x).double(), torch.from_numpy(y).double(), net64)
    loss.backward()
    lr = 1e-2
    t.fine_tune_compressed(data, test, epochs=1, learning_rate=lr)
    names = {layer: name for name, layer in t.neural_network.get_config().items()}
    assert {ti for (_, ti) in c0} == {0, 1}                  # quantized kernels and quantized biases both
    for (layer, ti), c in c0.items():
        p64 = list(getattr(net64, names[layer]).parameters())[ti]
        grad = p64.grad.numpy().ravel()
        dc64 = np.bincount(labels[(layer, ti)], weights=grad, minlength=c.size)
        mag = np.bincount(labels[(layer, ti)], weights=np.abs(grad), minlength=c.size)
        want = c.astype(np.float64) - lr * dc64
        got = models[layer][ti].cluster_centers_.ravel().astype(np.float64)
        assert np.all(np.abs(got - want) <= lr * (1e-4 * mag + 1e-9) + 2 * ref.U * np.abs(want)), (names[layer], ti)


def test_fine_tune_compressed_lowers_the_loss_and_keeps_the_indices(env, tmp_path):
    ops, _ = env
    from neural_network_compression_amd import compressed

    t, tr = _lenet300()
    data, test, x, y = _data(tr, 2048)
    t._prune_parameters(True)
    t.quantize(test, False, 4, "linear")
    models = t.quantized_models_by_layer
    lab0 = {(layer, ti): m.labels_compact_.clone() for layer, ms in models.items() for ti, m in enumerate(ms) if m is not None}
    raw0 = {(layer, ti): w.clone() for layer, ms in models.items() for ti, (w, m) in enumerate(zip(layer.get_weights(), ms)) if m is None}
    xb, yb = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    with torch.no_grad():
        loss0 = float(t._get_error(xb, yb))
    acc = t.fine_tune_compressed(data, test, epochs=2, learning_rate=1e-3)
    assert len(acc) == 2 and all(0.0 <= a <= 1.0 for a in acc)
    with torch.no_grad():
        loss1 = float(t._get_error(xb, yb))
    assert loss1 < loss0, (loss0, loss1)
    for layer, ms in models.items():
        for ti, (w, m) in enumerate(zip(layer.get_weights(), ms)):
            if m is None:
                assert torch.equal(w, raw0[(layer, ti)])
                continue
            assert torch.equal(m.labels_compact_, lab0[(layer, ti)])
            cen = torch.from_numpy(np.ascontiguousarray(m.cluster_centers_.ravel(), dtype=np.float32)).cuda()
            assert torch.equal(w.reshape(-1), ops.gather(cen, m.labels_compact_))
    net = t.compressed_network(trainable=True)
    assert all(isinstance(getattr(net, n), compressed.TrainableCompressedDense) for n in ("dense1", "dense2", "out"))
    # the trainers' L2 term from the codebook equals the float one to rounding
    for n in ("dense1", "dense2", "out"):
        a, b = float(getattr(net, n).kernel_sq_sum()), float((getattr(t.neural_network, n).kernel.double() ** 2).sum())
        assert abs(a - b) <= 1e-5 * b
    t.store_compressed(str(tmp_path))
    loaded = compressed.load_network(str(tmp_path / "weights.nnc"), t.neural_network)
    with torch.no_grad():
        assert torch.equal(net(xb[:300]), loaded(xb[:300]))


def test_lenet5_fine_tunes_through_its_conv_layers(env):
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
    before = {n: t.quantized_models_by_layer[getattr(t.neural_network, n)][0].cluster_centers_.copy() for n in ("conv1", "conv2")}
    net = t.compressed_network(trainable=True)
    assert isinstance(net.conv1, compressed.TrainableCompressedConv2D) and isinstance(net.conv2, compressed.TrainableCompressedConv2D)
    acc = t.fine_tune_compressed(data, test, epochs=1, learning_rate=1e-2)
    assert len(acc) == 1
    for n, c in before.items():
        after = t.quantized_models_by_layer[getattr(t.neural_network, n)][0].cluster_centers_
        assert not np.array_equal(after, c), n


def test_float_network_error_is_unchanged(env):
    """_get_error on the float network: the kernel_l2 helper forms exactly the old expression."""
    t, tr = _lenet300()
    _, _, x, y = _data(tr, 64)
    xb, yb = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    net = t.neural_network
    logits = net(xb)
    old = torch.nn.functional.binary_cross_entropy_with_logits(logits, yb) + 0.01 * sum(
        (layer.kernel ** 2).sum() / 2 for layer in (net.dense1, net.dense2, net.out))
    assert torch.equal(t._get_error(xb, yb), old)
