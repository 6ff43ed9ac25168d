"""Training group-wise codebook layers from their 2- and 4-bit packed indices (compressed.TrainableGroupedPackedCompressedDense,
compress_network_trainable_grouped(packed=), Trainer.fine_tune_grouped(packed=); run with -m gpu):
LeNet-300-100 quantized with group_rows = 32 (4 bits, linear) on a small synthetic data set, one batch of 512 per epoch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_compression_amd import synth  # noqa: E402
from tests.helpers import cbgrad_ref, grouped_grad_ref as ref  # noqa: E402

GR, LR, BITS = 32, 1e-2, 4
DENSE = ("dense1", "dense2", "out")


@pytest.fixture(scope="module")
def mods():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, compressed, ops
    from neural_network_compression_amd.common import utility

    _native.load()
    return ops, compressed, utility


def _trainer(seed=0):
    from neural_network_compression_amd.common import trainer as tr
    from neural_network_compression_amd.le_net_300_100_trainer import LeNet300100Trainer

    tr.Trainer.pruned_indexes_by_layer.clear()
    torch.manual_seed(seed)
    t = LeNet300100Trainer()
    layers = [layer for layer in t.neural_network.get_config().values() if layer.get_weights()]
    for li, ((_, wshape, bshape), layer) in enumerate(zip(synth.LENET_300_100, layers)):
        layer.set_weights([torch.from_numpy(synth.weights(wshape, 2000 + 2 * li)).cuda(), torch.from_numpy(synth.weights(bshape, 2001 + 2 * li)).cuda()])
    return t


def _data(n=512, seed=1):
    from neural_network_compression_amd.common import trainer as tr

    rng = np.random.RandomState(seed)
    x = rng.rand(n, 784).astype(np.float32)
    y = np.eye(10, dtype=np.float32)[rng.randint(0, 10, size=n)]
    return tr.LeNetDataset(x, y), tr.LeNetDataset(x[:128], y[:128].argmax(1)), x, y


def _decode(ops, wm, shape):
    """The float kernel of a GroupedModel: every group's own centres gathered by its own indices."""
    parts = [ops.gather(torch.from_numpy(np.ascontiguousarray(gm.cluster_centers_.ravel(), dtype=np.float32)).cuda(), gm.labels_compact_)
             for gm in wm.models]
    return torch.cat(parts).view(shape)


@pytest.fixture(scope="module")
def tuned300(mods):
    """LeNet-300-100 with group_rows = 32 after one epoch (one batch) of fine_tune_grouped(packed=True), with what it started
    from: the centres, the float64 gradients of the first batch on the decoded network, and the trainable networks."""
    ops, compressed, utility = mods
    t = _trainer()
    data, test, x, y = _data()
    t.quantize(test, False, 4, "linear", group_rows=GR)
    models = t.quantized_models_by_layer
    net_cfg = t.neural_network.get_config()
    start = {}
    for name in DENSE:
        wm, bm = models[net_cfg[name]]
        start[name] = dict(c=wm.cluster_centers_.copy(), lab=wm.labels_compact_.cpu().numpy().astype(np.int64), sizes=[int(m.cluster_centers_.size) for m in wm.models],
                           bc=None if bm is None else bm.cluster_centers_.ravel().copy(), blab=None if bm is None else bm.labels_compact_.cpu().numpy().astype(np.int64))
    before = t.compressed_network()
    nets = {p: compressed.compress_network_trainable_grouped(t.neural_network, models, packed=p) for p in (False, True, "auto")}
    nets["default"] = compressed.compress_network_trainable_grouped(t.neural_network, models)
    xb = torch.from_numpy(x).cuda()
    with torch.no_grad():
        inference = compressed.pack_grouped_layers(before)       # the same packed rows and kernels, inference only
        same_bits = torch.equal(nets[True](xb[:40]), inference(xb[:40])) and torch.equal(nets[True](xb[:7]), inference(xb[:7]))
    ws = [net_cfg[n].kernel.detach().double().cpu().requires_grad_(True) for n in DENSE]
    bs = [net_cfg[n].bias.detach().double().cpu().requires_grad_(True) for n in DENSE]
    a, xs, zs = torch.from_numpy(x).double(), [], []
    for i, (w, b) in enumerate(zip(ws, bs)):
        xs.append(a)
        z = a @ w + b
        z.retain_grad()
        zs.append(z)
        a = torch.relu(z) if i < 2 else z
    loss = torch.nn.functional.binary_cross_entropy_with_logits(a, torch.from_numpy(y).double()) + 0.01 * sum((w ** 2).sum() / 2 for w in ws)
    loss.backward()
    f64 = {n: dict(x=xs[i].detach().numpy(), g=zs[i].grad.numpy(), dw=ws[i].grad.numpy(), db=bs[i].grad.numpy()) for i, n in enumerate(DENSE)}
    built = []
    real = compressed.compress_network_trainable_grouped

    def spy(*a, **k):
        built.append((real(*a, **k), k))
        return built[-1][0]

    compressed.compress_network_trainable_grouped = spy
    try:
        acc = t.fine_tune_grouped(data, test, epochs=1, learning_rate=LR, packed=True)
    finally:
        compressed.compress_network_trainable_grouped = real
    assert built[0][1] == dict(packed=True)
    return dict(t=t, acc=acc, start=start, f64=f64, net=built[0][0], nets=nets, before=before, same_bits=same_bits, x=xb)


def test_the_trainable_grouped_packed_network(mods, tuned300):
    ops, compressed, utility = mods
    net, byte = tuned300["nets"][True], tuned300["nets"][False]
    for name in DENSE:
        layer, twin = getattr(net, name), getattr(byte, name)
        kin, kout = layer.kdim, layer.ncols
        assert isinstance(layer, compressed.TrainableGroupedPackedCompressedDense) and isinstance(twin, compressed.TrainableGroupedCompressedDense), name
        assert isinstance(layer, compressed._TrainableCentres) and (layer.bits, layer.k, layer.group_rows) == (BITS, 16, GR)
        assert isinstance(layer.centers, torch.nn.Parameter) and layer.centers.shape == layer.counts.shape == (-(-kin // GR), 16)
        assert torch.equal(layer.counts, twin.counts) and int(layer.counts.sum()) == kin * kout
        assert torch.equal(layer.kernel_sq_sum(), twin.kernel_sq_sum())           # the byte grouped layer's, bit for bit
        # packed is the only index buffer: no kdim x ncols byte tensor among the buffers
        assert not hasattr(layer, "labels")
        assert layer.packed.numel() == ops.packed_nbytes(kin, kout, BITS)
        assert all(b.numel() < kin * kout or n == "packed" for n, b in layer.named_buffers())
        quantized_bias = tuned300["start"][name]["bc"] is not None         # (a bias too short for 16 centres stays raw, and frozen)
        assert (layer.bias_centers is not None) == quantized_bias and (layer.bias is None) == quantized_bias
        bias_bytes = layer.bias_labels.numel() * layer.bias_labels.element_size() + 4 * layer.bias_centers.numel() if quantized_bias else 4 * layer.bias.numel()
        assert layer.nbytes() == layer.packed.numel() + 4 * layer.centers.numel() + bias_bytes
        assert compressed.compressed_nbytes(layer) == layer.nbytes()
        bias_args = dict(bias_codes=(torch.zeros_like(layer.bias_centers), layer.bias_labels)) if quantized_bias else dict(bias=torch.zeros_like(layer.bias))
        again = compressed.TrainableGroupedPackedCompressedDense.from_codes(kin, kout, GR, torch.zeros(kin * kout, dtype=torch.uint8, device="cuda"),
                                                                            torch.zeros_like(layer.centers), activation=layer.activation, **bias_args)
        assert set(again.state_dict()) == set(layer.state_dict()) and "packed" in layer.state_dict()
        again.load_state_dict(layer.state_dict())                # the state round-trips
        with torch.no_grad():
            xin = torch.rand(9, kin, device="cuda")
            assert torch.equal(again(xin), layer(xin))
            assert torch.equal(again.counts, layer.counts)
    assert compressed.compressed_nbytes(net) == sum(getattr(net, n).nbytes() for n in DENSE) < compressed.compressed_nbytes(byte)
    assert tuned300["same_bits"]                                  # under no_grad: pack_grouped_layers(compressed_network())'s output, bit for bit


def test_the_constructors_agree_bit_for_bit(mods, tuned300):
    ops, compressed, utility = mods
    t = tuned300["t"]
    cfg = t.neural_network.get_config()
    grouped_net = t.compressed_network()                                     # (the centres as they stand: the tuned ones)
    packed_net = compressed.pack_grouped_layers(grouped_net)
    cls = compressed.TrainableGroupedPackedCompressedDense
    for name in ("dense1", "dense2"):
        wm, bm = t.quantized_models_by_layer[cfg[name]]
        grouped, packed = getattr(grouped_net, name), getattr(packed_net, name)
        assert isinstance(packed, compressed.GroupedPackedCompressedDense)
        a, b, c = cls.from_grouped(grouped), cls.from_grouped_packed(packed), cls.from_dense(cfg[name], wm, bm)
        assert b.packed.data_ptr() == packed.packed.data_ptr()               # the same buffer: nothing repacked
        assert torch.equal(a.packed, b.packed) and torch.equal(a.packed, c.packed)
        assert torch.equal(a.counts, b.counts) and torch.equal(a.counts, c.counts)
        assert a.bias_centers is None and not a.bias.requires_grad
        with torch.no_grad():
            xin = torch.rand(20, grouped.kdim, device="cuda")
            want = packed(xin)
            for layer in (a, b, c):
                assert torch.equal(layer(xin), want)


def test_the_packed_keyword(mods, tuned300):
    ops, compressed, utility = mods
    nets, t = tuned300["nets"], tuned300["t"]
    kinds = {p: [type(getattr(n, name)).__name__ for name in DENSE] for p, n in nets.items()}
    assert kinds[False] == kinds["default"] == ["TrainableGroupedCompressedDense"] * 3
    assert kinds[True] == ["TrainableGroupedPackedCompressedDense"] * 3
    # "auto": 100 x 10 at 4 bits is 100 rows of 16 bytes, more than its 1000 byte indices: it stays in the byte form
    assert ops.packed_nbytes(100, 10, 4) == 1600
    assert kinds["auto"] == ["TrainableGroupedPackedCompressedDense"] * 2 + ["TrainableGroupedCompressedDense"]
    sd_false, sd_default = nets[False].state_dict(), nets["default"].state_dict()
    assert list(sd_false) == list(sd_default) and all(torch.equal(sd_false[k], sd_default[k]) for k in sd_false)
    assert compressed.compressed_nbytes(nets["auto"]) < compressed.compressed_nbytes(nets[True]) < compressed.compressed_nbytes(nets[False])
    for bad in (None, "yes", 2, 0, 1):
        with pytest.raises(ValueError, match="packed"):
            compressed.compress_network_trainable_grouped(t.neural_network, t.quantized_models_by_layer, packed=bad)


def test_ungrouped_layers_stay_in_the_byte_trainable_forms(mods):
    ops, compressed, utility = mods
    _, test, _, _ = _data()
    t = _trainer(seed=4)
    t.quantize(test, False, 4, "linear")
    for packed in (True, "auto"):
        a = compressed.compress_network_trainable_grouped(t.neural_network, t.quantized_models_by_layer, packed=packed)
        b = compressed.compress_network_trainable(t.neural_network, t.quantized_models_by_layer)
        assert [type(m) for m in a.get_config().values()] == [type(m) for m in b.get_config().values()]


def test_one_batch_of_fine_tune_grouped_packed_is_the_float64_step(mods, tuned300):
    """got = c - lr * dc with dc the kernel's float32 (G, K) gradient plus autograd's L2 term 0.01 * counts * c.  The tolerance is
    that of the byte grouped layers' test: against float64 the kernel's error is dc_bound (S taken one lower than the float64
    maxima give, since the device takes it from its float32 ones); the x and g it is fed are float32 results of chains of at most
    784 + 300 + 100 + 16 operations each, 2 * 1200 u of the magnitude sum; the L2 term and the step round a few times more.  The
    derivation bounds chain lengths, not the order the kernels sum in, so it holds for the packed kernels unchanged."""
    ops, compressed, utility = mods
    t, start, f64 = tuned300["t"], tuned300["start"], tuned300["f64"]
    assert len(tuned300["acc"]) == 1 and 0.0 <= tuned300["acc"][0] <= 1.0
    assert all(isinstance(getattr(tuned300["net"], n), compressed.TrainableGroupedPackedCompressedDense) for n in DENSE)
    cfg = t.neural_network.get_config()
    u = cbgrad_ref.U
    for name in DENSE:
        wm, bm = t.quantized_models_by_layer[cfg[name]]
        kin, kout = cfg[name].kernel.shape
        case = dict(m=512, kdim=kin, ncols=kout, k=16, group_rows=GR, off=0)
        s, r = start[name], f64[name]
        lab = s["lab"].reshape(kin, kout)
        got = wm.cluster_centers_.astype(np.float64)
        assert got.shape == s["c"].shape and not np.array_equal(got, s["c"])            # the centres moved
        dc64 = np.stack([cbgrad_ref.bin64(r["dw"][ref.group_rows_of(case, q)], lab[ref.group_rows_of(case, q)], 16) for q in range(ref.groups_of(case))])
        tl = ops.cbpk_grouped_dc_plan(512, kin, kout, BITS, 16, GR, ops.device_info()[1])["terms_log2"]
        S, flag = ops.cbgrad_shift(512, np.abs(r["x"]).max(), np.abs(r["g"]).max(), tl)
        assert flag == ops.CBGRAD_OK
        x32, g32 = r["x"].astype(np.float32), r["g"].astype(np.float32)
        bound = ref.dc_bound(case, x32, g32, lab, S - 1, f32_out=True)
        mag = np.stack([cbgrad_ref.bin64(cbgrad_ref.dw64(np.abs(r["x"][:, ref.group_rows_of(case, q)]), np.abs(r["g"])), lab[ref.group_rows_of(case, q)], 16)
                        for q in range(ref.groups_of(case))])
        counts = np.stack([np.bincount(lab[ref.group_rows_of(case, q)].ravel(), minlength=16) for q in range(ref.groups_of(case))])
        l2 = 0.01 * counts * np.abs(s["c"].astype(np.float64))
        tol = bound + 2 * 1200 * u * mag + 8 * u * l2 + 4 * u * np.abs(dc64)
        want = s["c"].astype(np.float64) - LR * dc64
        err = np.abs(got - want)
        print(f"{name}: max |got - want| {err.max():.3e}, its tolerance {(LR * tol + 2 * u * np.abs(want))[np.unravel_index(err.argmax(), err.shape)]:.3e}, "
              f"max step {np.abs(LR * dc64).max():.3e}")
        assert np.all(err <= LR * tol + 2 * u * np.abs(want)), name
        if s["bc"] is None:
            assert bm is None
            continue
        dbc = np.bincount(s["blab"], weights=r["db"], minlength=s["bc"].size)
        bmag = np.bincount(s["blab"], weights=np.abs(f64[name]["g"]).sum(0), minlength=s["bc"].size)
        bwant = s["bc"].astype(np.float64) - LR * dbc
        assert np.all(np.abs(bm.cluster_centers_.ravel() - bwant) <= LR * (1e-4 * bmag + 1e-9) + 2 * u * np.abs(bwant)), name


def test_the_tuned_centres_go_back_everywhere(mods, tuned300):
    ops, compressed, utility = mods
    t, net = tuned300["t"], tuned300["net"]
    cfg = t.neural_network.get_config()
    after = t.compressed_network()
    packed_after = compressed.pack_grouped_layers(after)
    for name in DENSE:
        wm, _ = t.quantized_models_by_layer[cfg[name]]
        tuned = getattr(net, name).centers.detach()
        assert isinstance(getattr(after, name), compressed.GroupedCompressedDense)
        assert isinstance(getattr(packed_after, name), compressed.GroupedPackedCompressedDense)
        assert torch.equal(getattr(after, name).centers, tuned), name                   # compressed_network(): the tuned (G, K), bit for bit
        assert torch.equal(getattr(packed_after, name).centers, tuned), name
        assert torch.equal(getattr(packed_after, name).packed, getattr(net, name).packed), name
        assert np.array_equal(wm.cluster_centers_, tuned.cpu().numpy())
        for q, gm in enumerate(wm.models):                                              # each group's own model, not the padding
            assert gm.cluster_centers_.shape == (tuned300["start"][name]["sizes"][q], 1)
            assert np.array_equal(gm.cluster_centers_.ravel(), wm.cluster_centers_[q, : gm.cluster_centers_.size])
        assert torch.equal(cfg[name].kernel.detach(), _decode(ops, wm, cfg[name].kernel.shape)), name   # the float kernel is its decode
        assert torch.equal(wm.labels_compact_.cpu(), torch.from_numpy(tuned300["start"][name]["lab"].astype(np.uint8)))   # the indices stayed
    with torch.no_grad():
        x = tuned300["x"][:40]
        assert torch.equal(packed_after(x), net(x)) and torch.equal(packed_after(x[:7]), net(x[:7]))


def test_the_old_entry_points_keep_refusing_grouped_layers(mods, tuned300):
    ops, compressed, utility = mods
    t = tuned300["t"]
    data, test, _, _ = _data()
    for call in (lambda: t.fine_tune_compressed(data, test, 1), lambda: t.fine_tune_compressed(data, test, 1, packed=True),
                 lambda: t.fine_tune_centroids(data, test, 1), lambda: t.compressed_network(trainable=True),
                 lambda: compressed.compress_network_trainable(t.neural_network, t.quantized_models_by_layer),
                 lambda: compressed.compress_network_trainable(t.neural_network, t.quantized_models_by_layer, packed=True)):
        with pytest.raises(NotImplementedError, match="dense1"):
            call()
