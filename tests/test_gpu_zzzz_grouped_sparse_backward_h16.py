"""The backward pass of the pruned group-wise codebook layer on bf16 / fp16 activations from the bitmap-sparse form
(nnc_cbsp_grouped_dx_h16 / nnc_cbsp_grouped_dc_h16, csrc/nnc_cbspgrad_grouped_h16.hip) through the ops, the
trainable layer and Trainer.fine_tune_grouped (run with -m gpu).  Every assertion is an equality of bits.

The zero symbols differ between the groups; where a case has more than one group and K < 256, group 1 has z_q = K + 1 >= K (c_z = 0;
a uint8 symbol cannot reach K = 256, so the K = 256 case has none); the K = 16, four-table case and the last stream case store
symbols >= K.
(The file name sorts behind every earlier GPU test file, so the suite's order up to here is what it was.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# (m, kdim, ncols, K, group_rows, density)
CASES = [(17, 32, 1, 2, 32, 0.5),        # first row past the stream path, one column
         (33, 104, 65, 16, 32, 0.1),     # four tables in a tile, short last group of 8 rows, a column past a 64-bit segment, odd row pitch
         (40, 160, 200, 17, 64, 0.1),    # second index-row tile starts at group 2; dx splits 3 x 96 columns, the last split 8 wide
         (129, 300, 63, 256, 96, 0.3),   # two m tiles, groups unaligned with the 128-row tile, K = 256, dc split 96 + 33 rows
         (20, 256, 64, 16, 128, 0.0),    # nnz = 0, one table per tile, vector-load arm
         (20, 64, 128, 4, 32, 1.0),      # every weight stored
         (16, 104, 65, 16, 32, 0.1),     # stream path at MT edge, short last group
         (3, 104, 65, 16, 32, 0.1),      # ... and below
         (16, 104, 200, 16, 32, 0.1)]    # beside the issue's list: two column blocks at m = 16, so the half stream dx writes split partials
IDS = ["m%d-kd%d-n%d-k%d-gr%d-d%g" % c for c in CASES]
DTYPES = [torch.bfloat16, torch.float16]
DT_CODE = {torch.bfloat16: 1, torch.float16: 2}
PAD = 64


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, ops

    _native.load()
    return ops


def _labels(case, seed):
    """(labels (kdim, ncols), zero symbols (G,)): a weight is stored (its label differs from its group's z_q) with the case's density."""
    m, kdim, ncols, k, gr, density = case
    rng = np.random.RandomState(seed)
    G = -(-kdim // gr)
    zs = ((1 + 2 * np.arange(G)) % k).astype(np.uint8)
    if G > 1 and k < 255:
        zs[1] = k + 1
    z = np.repeat(zs.astype(np.int64), gr)[:kdim, None]
    r = rng.randint(0, k - 1, size=(kdim, ncols))
    stored = np.where(z < k, r + (r >= z), rng.randint(0, k, size=(kdim, ncols)))   # a label of the codebook other than z_q
    if case in (CASES[1], CASES[8]):
        stored[rng.rand(kdim, ncols) < 0.2] = k + 3                                   # stored symbols >= K, on the MFMA and the stream path
    lab = np.where(rng.rand(kdim, ncols) < density, stored, z)
    return lab, zs


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(dtype)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def forms(ops):
    """Per case, made once and left unchanged: the labels, the zero symbols, the packed form and its unpacked labels."""
    out = {}
    for ci, case in enumerate(CASES):
        m, kdim, ncols, k, gr, density = case
        lab, zs = _labels(case, 50 + ci)
        lab_t = torch.from_numpy(lab.astype(np.uint8).ravel()).cuda()
        codes = ops.pack_grouped_sparse_codes(lab_t, kdim, ncols, k, gr, zero_symbols=torch.from_numpy(zs).cuda())
        assert codes.nnz == int((lab != np.repeat(zs.astype(np.int64), gr)[:kdim, None]).sum())
        assert (codes.nnz == 0) == (density == 0) and (codes.nnz == kdim * ncols) == (density == 1)
        dense = codes.to_dense()
        assert np.array_equal(dense.cpu().numpy().reshape(lab.shape), lab)
        out[case] = dict(lab=lab, zs=zs, codes=codes, dense=dense)
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_data_is_the_float64_formula(ops, forms, case, dt):
    """x and g are integers in [-2, 2], the centres quarter-integers in [-2, 2] (exact in bf16): every float64 sum is a multiple of
    1/4 below 2^22, so exact in float32, and dW is an integer, exact on the plan's fixed-point grid wherever its shift S >= 0."""
    m, kdim, ncols, k, gr, _ = case
    f = forms[case]
    rng = np.random.RandomState(m + kdim)
    x, g = rng.randint(-2, 3, size=(m, kdim)).astype(np.float64), rng.randint(-2, 3, size=(m, ncols)).astype(np.float64)
    G = len(f["zs"])
    cen = rng.randint(-8, 9, size=(G, k)) / 4.0
    q = np.arange(kdim)[:, None] // gr
    lab = f["lab"]
    W = np.where(lab < k, cen[q, np.minimum(lab, k - 1)], 0.0)
    want_dx = g @ W.T
    dW = x.T @ g
    want_dc = np.zeros((G, k))
    np.add.at(want_dc, (np.broadcast_to(q, lab.shape)[lab < k], lab[lab < k]), dW[lab < k])
    S, flag = ops.cbgrad_shift(m, np.abs(x).max(), np.abs(g).max(), ops.cbsp_grouped_dc_h16_plan(dt, m, kdim, ncols, k, gr, ops.device_info()[1])["terms_log2"])
    assert flag == ops.CBGRAD_OK and S >= 0 and np.abs(want_dx * 4).max() < 2 ** 24 and np.abs(want_dc).max() < 2 ** 24   # the precondition
    xt, gt, ct = _dev(x, dt), _dev(g, dt), _dev(cen)
    dx32 = ops.grouped_sparse_codebook_matmul_dx(gt, f["codes"], ct, out_dtype=torch.float32, half_inputs=True)
    dx = ops.grouped_sparse_codebook_matmul_dx(gt, f["codes"], ct, half_inputs=True)
    assert _same(dx32, _dev(want_dx)) and _same(dx, _dev(want_dx).to(dt))
    dc = ops.grouped_sparse_codebook_centroid_grad(xt, gt, f["codes"], half_inputs=True)
    dc32 = ops.grouped_sparse_codebook_centroid_grad(xt, gt, f["codes"], dtype=torch.float32, half_inputs=True)
    assert dc.dtype == torch.float64 and np.array_equal(dc.cpu().numpy(), want_dc)
    assert np.array_equal(dc32.cpu().numpy(), want_dc.astype(np.float32))


def _raw(ops, case, dt, f, xt, gt, ct):
    """The native calls on outputs and workspaces framed by sentinels -> (dx, dx32, dc, dc32) once nothing outside them was written."""
    from neural_network_compression_amd import _native as nat

    L = nat.load()
    m, kdim, ncols, k, gr, _ = case
    codes, G, code, s = f["codes"], len(f["zs"]), DT_CODE[dt], torch.cuda.current_stream().cuda_stream
    outs = []

    def framed(nbytes):
        buf = torch.full((PAD + nbytes + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        return buf, buf[PAD: PAD + nbytes]

    def intact(buf, nbytes):
        return bool((buf[:PAD] == 0xA5).all()) and bool((buf[PAD + nbytes:] == 0xA5).all())

    for out_code, tdt in ((code, dt), (0, torch.float32)):
        nb, ws_bytes = m * kdim * (4 if out_code == 0 else 2), int(L.nnc_cbsp_grouped_dx_h16_workspace_bytes(m, kdim, ncols))
        (dbuf, dx), (wbuf, ws) = framed(nb), framed(ws_bytes)
        nat.check(L.nnc_cbsp_grouped_dx_h16(gt.data_ptr(), code, m, kdim, codes.buf.data_ptr(), codes.buf.numel(), ncols, codes.zero_symbols.data_ptr(),
                                            codes.nnz, ct.data_ptr(), k, gr, dx.data_ptr(), out_code, ws.data_ptr() if ws_bytes else None, ws_bytes, s))
        torch.cuda.synchronize()
        assert intact(dbuf, nb) and intact(wbuf, ws_bytes)
        outs.append(dx.view(tdt).view(m, kdim).clone())
    for f64, tdt in ((1, torch.float64), (0, torch.float32)):
        nb, ws_bytes = G * k * (8 if f64 else 4), int(L.nnc_cbsp_grouped_dc_h16_workspace_bytes(m, kdim, ncols, k, gr))
        assert ws_bytes == 64 + 8 * G * k
        (dbuf, dc), (wbuf, ws) = framed(nb), framed(ws_bytes)
        nat.check(L.nnc_cbsp_grouped_dc_h16(xt.data_ptr(), gt.data_ptr(), code, m, kdim, codes.buf.data_ptr(), codes.buf.numel(), ncols,
                                            codes.zero_symbols.data_ptr(), codes.nnz, k, gr, dc.data_ptr(), f64, ws.data_ptr(), ws_bytes, s))
        torch.cuda.synchronize()
        assert intact(dbuf, nb) and intact(wbuf, ws_bytes)
        outs.append(dc.view(tdt).view(G, k).clone())
    return outs


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_identities_on_normal_data_and_a_second_call_inside_sentinel_frames(ops, forms, case, dt):
    m, kdim, ncols, k, gr, _ = case
    f = forms[case]
    codes, dense = f["codes"], f["dense"]
    rng = np.random.RandomState(7 * m + ncols)
    xt, gt = _dev(rng.standard_normal((m, kdim)), dt), _dev(rng.standard_normal((m, ncols)), dt)
    ct = _dev(rng.standard_normal((len(f["zs"]), k)))
    dx = ops.grouped_sparse_codebook_matmul_dx(gt, codes, ct, half_inputs=True)
    dx32 = ops.grouped_sparse_codebook_matmul_dx(gt, codes, ct, out_dtype=torch.float32, half_inputs=True)
    dc = ops.grouped_sparse_codebook_centroid_grad(xt, gt, codes, half_inputs=True)
    dc32 = ops.grouped_sparse_codebook_centroid_grad(xt, gt, codes, dtype=torch.float32, half_inputs=True)
    assert dx.dtype == dt and dx32.dtype == torch.float32 and bool(dx32.any())
    if m > 16:
        assert _same(dx, ops.grouped_codebook_matmul_dx(gt, dense, ct, kdim, ncols, gr))
        assert _same(dx32, ops.grouped_codebook_matmul_dx(gt, dense, ct, kdim, ncols, gr, out_dtype=torch.float32))
    else:
        assert _same(dx32, ops.grouped_sparse_codebook_matmul_dx(gt.float(), codes, ct.to(dt).float()))
        assert _same(dx, dx32.to(dt))
    assert _same(dc, ops.grouped_codebook_centroid_grad(xt, gt, dense, k, kdim, ncols, gr))
    assert _same(dc32, ops.grouped_codebook_centroid_grad(xt, gt, dense, k, kdim, ncols, gr, dtype=torch.float32))
    for got, want in zip(_raw(ops, case, dt, f, xt, gt, ct), (dx, dx32, dc, dc32)):   # a second, identical call: the same bits
        assert _same(got, want)


@pytest.mark.parametrize("dt", DTYPES, ids=["bf16", "fp16"])
def test_one_training_step_is_the_byte_grouped_layers(ops, forms, dt):
    """m = 40 > 16: the sparse half forward is the byte grouped one bit for bit, so both layers see the same g, and dx and dc are equal
    bit for bit: after one step the centres and the quantized bias's centres of the two layers have the same bits."""
    from neural_network_compression_amd import compressed

    case = CASES[2]
    m, kdim, ncols, k, gr, _ = case
    f = forms[case]
    rng = np.random.RandomState(3)
    cen, x, gy = rng.standard_normal((len(f["zs"]), k)), rng.standard_normal((m, kdim)), rng.standard_normal((m, ncols))
    bias = (_dev(rng.standard_normal(8) * 0.1), torch.from_numpy((np.arange(ncols) % 8).astype(np.uint8)).cuda())
    byte = compressed.TrainableGroupedCompressedDense.from_codes(kdim, ncols, gr, f["dense"], _dev(cen), None, bias, torch.relu, half_inputs=True)
    sparse = compressed.TrainableGroupedSparseCompressedDense.from_codes(kdim, ncols, gr, f["dense"], _dev(cen), None, bias, torch.relu,
                                                                         zero_symbols=f["codes"].zero_symbols, half_inputs=True)
    assert sparse.half_inputs and sparse.nnz == f["codes"].nnz
    tuned = []
    for layer in (byte, sparse):
        xt = _dev(x, dt).requires_grad_(True)
        y = layer(xt)
        assert y.dtype == dt
        y.backward(_dev(gy, dt))
        with torch.no_grad():
            tuned.append([y.detach(), xt.grad] + [p - 1e-2 * p.grad for p in (layer.centers, layer.bias_centers)])
        assert layer.centers.grad.dtype == torch.float32 and bool(layer.centers.grad.any())
    assert all(_same(a, b) for a, b in zip(*tuned))


def test_one_epoch_of_fine_tune_grouped_on_a_pruned_network_in_bf16(ops):
    from neural_network_compression_amd import synth
    from neural_network_compression_amd.common import trainer as tr
    from neural_network_compression_amd.le_net_300_100_trainer import LeNet300100Trainer

    tr.Trainer.pruned_indexes_by_layer.clear()
    torch.manual_seed(0)
    t = LeNet300100Trainer()
    layers = [layer for layer in t.neural_network.get_config().values() if layer.get_weights()]
    for li, ((_, wshape, bshape), layer) in enumerate(zip(synth.LENET_300_100, layers)):
        layer.set_weights([torch.from_numpy(synth.weights(wshape, 2000 + 2 * li)).cuda(), torch.from_numpy(synth.weights(bshape, 2001 + 2 * li)).cuda()])
    rng = np.random.RandomState(1)
    x = rng.rand(512, 784).astype(np.float32)
    y = np.eye(10, dtype=np.float32)[rng.randint(0, 10, size=512)]
    data, test = tr.LeNetDataset(x, y), tr.LeNetDataset(x[:128], y[:128].argmax(1))
    t._prune_parameters(True)
    t.quantize(test, False, 4, "linear", group_rows=32)
    models, cfg = t.quantized_models_by_layer, t.neural_network.get_config()
    names = [n for n, layer in cfg.items() if models.get(layer)]
    before = {n: models[cfg[n]][0].cluster_centers_.copy() for n in names}
    acc = t.fine_tune_grouped(data, test, epochs=1, learning_rate=1e-2, sparse=True, activation_dtype=torch.bfloat16, sparse_half_inputs=True)
    assert len(acc) == 1 and 0.0 <= acc[0] <= 1.0
    after = t.compressed_network()
    for n in names:
        tuned = models[cfg[n]][0].cluster_centers_
        assert np.isfinite(tuned).all() and not np.array_equal(tuned, before[n])                      # the tuned centres, written back
        assert np.array_equal(getattr(after, n).centers.cpu().numpy(), tuned.astype(np.float32))      # and visible in compressed_network()
