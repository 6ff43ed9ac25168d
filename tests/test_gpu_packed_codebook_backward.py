"""The backward pass of the 2- and 4-bit packed codebook matmul (nnc_cbpk_dx_f32 / nnc_cbpk_dc_f32, csrc/nnc_cbpkgrad.hip), the
autograd Function ops.packed_codebook_linear, the trainable packed layers, compress_network_trainable(packed=...) and
Trainer.fine_tune_compressed(packed=...) (run with -m gpu).

The centroid gradient must equal the byte backward's on the unpacked labels bit for bit in every regime of both plans, which the
case list is asserted to cover at the device's CU count, at every scale of x and g; exact data must give the dx formula bit for
bit; the padding of a row is never read as a weight nor binned; fitted layers stay within the float32 bound of DESIGN.md section
12; the backward reads nothing back and allocates no kdim x ncols tensor."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_compression_amd import synth  # noqa: E402
from tests.helpers import cbgrad_ref, packed_ref  # noqa: E402
from tests.helpers import packed_grad_ref as ref  # noqa: E402
from tests.helpers import range_ref as rr  # noqa: E402

LIVE_CASES = [c for c in ref.CASES if c[1] * c[2] * c[3] > 0]


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, ops

    _native.load()
    _, cus = ops.device_info()
    return ops, cus


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dev_labels(lab):
    return torch.from_numpy(np.ascontiguousarray(lab, dtype=np.uint8).ravel()).cuda()


def _codes(ops, lab, bits, k):
    kdim, ncols = lab.shape
    codes = ops.pack_codes(_dev_labels(lab), kdim, ncols, k, bits)
    assert np.array_equal(codes.packed.cpu().numpy(), packed_ref.pack(lab, kdim, ncols, bits))
    return codes


def _case(ops, case, seed):
    _, m, kdim, ncols, bits, k = case
    x, g, c, lab = ref.case_data(case, seed)
    return x, g, c, lab, _codes(ops, lab, bits, k)


def _seed(case):
    return len(case[0]) * 7 + case[1]


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0)) and torch.equal(torch.isnan(a), torch.isnan(b))


def test_every_regime_is_covered_at_this_cu_count(env):
    ops, cus = env
    ref.assert_covered(ops, cus)


@pytest.mark.parametrize("case", ref.CASES, ids=[c[0] for c in ref.CASES])
def test_exact_data_dx_formula_and_dc_of_the_byte_backward(env, case):
    ops, cus = env
    name, m, kdim, ncols, bits, k = case
    x, g, c, lab, codes = _case(ops, case, _seed(case))
    if k < (1 << bits) and lab.size:
        assert (lab >= k).any()                              # labels >= K occur
    xt, gt, ct = _cuda(x), _cuda(g), _cuda(c)
    dx = ops.packed_codebook_matmul_dx(gt, codes, ct)
    assert dx.shape == (m, kdim) and dx.dtype == torch.float32
    want = ref.dx64(g, lab, c, bits)
    print(name, "dx max |got - formula| =", float(np.abs(dx.cpu().numpy() - want).max()) if want.size else 0.0)
    assert np.array_equal(dx.cpu().numpy(), want), name
    byte_labels = codes.to_dense()
    for dt in (torch.float64, torch.float32):
        dc = ops.packed_codebook_centroid_grad(xt, gt, codes, dtype=dt)
        byte = ops.codebook_centroid_grad(xt, gt, byte_labels, k, kdim, ncols, dtype=dt)
        assert dc.dtype == dt and dc.shape == (k,) and torch.equal(dc, byte), name
        assert np.array_equal(dc.cpu().numpy(), ref.dc64(x, g, lab, k, bits).astype(dc.cpu().numpy().dtype)), name
    # a second call gives the same bits
    assert torch.equal(ops.packed_codebook_matmul_dx(gt, codes, ct), dx)
    assert torch.equal(ops.packed_codebook_centroid_grad(xt, gt, codes), ops.packed_codebook_centroid_grad(xt, gt, codes))


@pytest.mark.parametrize("m", [4, 40])
@pytest.mark.parametrize("bits,k", [(2, 3), (4, 16)])
def test_dc_all_nan_and_zero_cases_match_the_byte_backward(env, m, bits, k):
    ops, _ = env
    rng = np.random.RandomState(m + bits)
    kdim, ncols = 70, 130
    lab = rng.randint(0, 1 << bits, size=(kdim, ncols))
    codes = _codes(ops, lab, bits, k)
    byte_labels = codes.to_dense()
    x = rng.randn(m, kdim).astype(np.float32)
    g = rng.randn(m, ncols).astype(np.float32)
    x_nan, g_inf = x.copy(), g.copy()
    x_nan[1, 3] = np.nan
    g_inf[0, 129] = np.inf
    big = np.float32(2.0 ** 63)
    cases = {"nan_in_x": (x_nan, g, "nan"), "inf_in_g": (x, g_inf, "nan"), "bound_beyond_2^127": (x * big, g * big, "nan"),
             "zero_g": (x, np.zeros_like(g), "zero"), "zero_x": (np.zeros_like(x), g, "zero"), "plain": (x, g, "finite")}
    for what, (xx, gg, kind) in cases.items():
        xt, gt = _cuda(xx), _cuda(gg)
        for dt in (torch.float64, torch.float32):
            got = ops.packed_codebook_centroid_grad(xt, gt, codes, dtype=dt)
            byte = ops.codebook_centroid_grad(xt, gt, byte_labels, k, kdim, ncols, dtype=dt)
            assert _same(got, byte), what
            h = got.cpu().numpy()
            if kind == "nan":
                assert np.isnan(h).all(), what
            elif kind == "zero":
                assert (h == 0).all() and not np.signbit(h).any(), what
            else:
                assert np.isfinite(h).all() and h.any(), what


def _scaled_dc_is_the_byte_dc_and_the_formula(ops, case, a, b):
    name, m, kdim, ncols, bits, k = case
    xi, gi, _, lab, codes = _case(ops, case, _seed(case))
    x, g = rr.scale(xi, a), rr.scale(gi, b)
    xt, gt = _cuda(x), _cuda(g)
    byte_labels = codes.to_dense()
    f64 = ref.dc64(x, g, lab, k, bits)
    for dt in (torch.float64, torch.float32):
        got = ops.packed_codebook_centroid_grad(xt, gt, codes, dtype=dt)
        assert torch.equal(got, ops.codebook_centroid_grad(xt, gt, byte_labels, k, kdim, ncols, dtype=dt)), (name, a, b)
        want = f64 if dt == torch.float64 else rr.f32_of(f64)
        assert np.array_equal(got.cpu().numpy(), want), (name, a, b)


@pytest.mark.parametrize("ab", [e for e in rr.DC_EXPONENTS if e[0] in ("below_denorm_100", "subnormal_x", "large")], ids=lambda e: e[0])
@pytest.mark.parametrize("case", LIVE_CASES, ids=[c[0] for c in LIVE_CASES])
def test_dc_is_the_byte_dc_and_the_formula_at_every_scale(env, case, ab):
    ops, _ = env
    _scaled_dc_is_the_byte_dc_and_the_formula(ops, case, ab[1], ab[2])


@pytest.mark.parametrize("case", LIVE_CASES, ids=[c[0] for c in LIVE_CASES])
def test_dc_just_below_the_top_of_the_range(env, case):
    ops, _ = env
    xi, gi, _, _ = ref.case_data(case, _seed(case))
    e = rr.top_exponent(case[1], xi, gi, below=True)
    _scaled_dc_is_the_byte_dc_and_the_formula(ops, case, e // 2, e - e // 2)


def _framed(host):
    """A contiguous misaligned view (buf[1:1 + n]) of a buffer that holds NaN before and after it."""
    host = np.ascontiguousarray(host, dtype=np.float32)
    buf = torch.full((host.size + 64,), float("nan"), dtype=torch.float32, device="cuda")
    buf[1:1 + host.size] = torch.from_numpy(host.ravel()).cuda()
    return buf[1:1 + host.size].view(host.shape)


@pytest.mark.parametrize("m", [1, 5, 16, 40])
@pytest.mark.parametrize("ncols", [7, 33, 50, 1027])
@pytest.mark.parametrize("bits,k", [(2, 4), (4, 16), (4, 3)])
def test_padding_is_neither_a_weight_nor_binned(env, m, ncols, bits, k):
    """A padding field is label 0 and c[0] != 0: neither it nor a lane past ncols may meet what lies after a row of g, nor fall
    into bin 0."""
    ops, _ = env
    rng = np.random.RandomState(1000 * m + ncols + bits)
    kdim = 45
    lab = rng.randint(0, 1 << bits, size=(kdim, ncols))
    c = (rng.randint(1, 9, size=k) / 4.0).astype(np.float32)          # c[0] != 0
    x = rng.randint(-3, 4, size=(m, kdim)).astype(np.float32)
    g = rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
    codes = _codes(ops, lab, bits, k)
    xt, gt, ct = _framed(x), _framed(g), _cuda(c)
    assert xt.data_ptr() % 8 == 4 and gt.is_contiguous()
    dx = ops.packed_codebook_matmul_dx(gt, codes, ct).cpu().numpy()
    assert np.isfinite(dx).all() and np.array_equal(dx, ref.dx64(g, lab, c, bits))
    for dt in (torch.float64, torch.float32):
        dc = ops.packed_codebook_centroid_grad(xt, gt, codes, dtype=dt)
        want = ref.dc64(x, g, lab, k, bits)
        assert np.array_equal(dc.cpu().numpy(), want.astype(dc.cpu().numpy().dtype)), (dc[0], want[0])
        assert torch.equal(dc, ops.codebook_centroid_grad(xt, gt, codes.to_dense(), k, kdim, ncols, dtype=dt))


@functools.lru_cache(maxsize=None)
def _fit(shape, seed, bits):
    from neural_network_compression_amd import pipeline

    w = synth.weights(shape, seed)
    res = pipeline.compress_layer(torch.from_numpy(w.copy()).cuda(), q=1, bits=bits, mode="linear")
    return res.model.cluster_centers_.ravel().astype(np.float32), res.model.labels_.reshape(shape).astype(np.int64)


FIT_SHAPES = [(int(np.prod(s[:-1])), s[-1]) for _, s, _ in synth.LENET_300_100 + synth.LENET_5]      # (a conv kernel as its patch matrix)


@pytest.mark.parametrize("m", [1, 16, 256])
@pytest.mark.parametrize("bits", [2, 4])
@pytest.mark.parametrize("shape", FIT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fitted_layers_are_within_the_dx_bound_and_dc_is_the_byte_dc(env, m, bits, shape):
    ops, cus = env
    c, lab = _fit(tuple(shape), 7000 + bits, bits)
    assert c.size == 1 << bits
    kdim, ncols = shape
    codes = _codes(ops, lab, bits, c.size)
    rng = np.random.RandomState(m)
    x = (rng.randn(m, kdim) * 0.7).astype(np.float32)
    g = (rng.randn(m, ncols) * 1e-2).astype(np.float32)
    xt, gt = _cuda(x), _cuda(g)
    dx = ops.packed_codebook_matmul_dx(gt, codes, _cuda(c)).cpu().numpy()
    want, bound = ref.dx_bound(g, lab, c)
    print(shape, bits, m, "dx max err / bound =", float((np.abs(dx - want) / bound).max()))
    assert np.all(np.abs(dx - want) <= bound)
    byte_labels = codes.to_dense()
    t = ops.cbpk_dc_plan(m, kdim, ncols, bits, c.size, cus)["terms_log2"]
    S, flag = ops.cbgrad_shift(m, float(np.abs(x).max()), float(np.abs(g).max()), t)
    assert flag == ops.CBGRAD_OK
    for dt in (torch.float64, torch.float32):
        dc = ops.packed_codebook_centroid_grad(xt, gt, codes, dtype=dt)
        assert torch.equal(dc, ops.codebook_centroid_grad(xt, gt, byte_labels, c.size, kdim, ncols, dtype=dt))
        err = np.abs(dc.cpu().numpy().astype(np.float64) - cbgrad_ref.dc64(x, g, lab, c.size))
        assert np.all(err <= cbgrad_ref.dc_bound(x, g, lab, c.size, S, f32_out=dt == torch.float32) + 1e-300)


# ------------------------------------------------------------------ autograd
def _layer_data(ops, m, seed, kdim=90, ncols=150, bits=4, k=13, exact=False):
    rng = np.random.RandomState(seed)
    lab = rng.randint(0, 1 << bits, size=(kdim, ncols))
    if exact:
        x = rng.randint(-3, 4, size=(m, kdim)).astype(np.float32)
        c = (rng.randint(-8, 9, size=k) / 4.0).astype(np.float32)
        b = rng.randint(-3, 4, size=ncols).astype(np.float32)
        w = rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
    else:
        x = (rng.randn(m, kdim) * 0.5).astype(np.float32)
        c = (rng.randn(k) * 0.1).astype(np.float32)
        b = (rng.randn(ncols) * 0.1).astype(np.float32)
        w = rng.randn(m, ncols).astype(np.float32)
    codes = _codes(ops, lab, bits, k)
    return x, c, lab, b, w, codes.to_dense(), codes


def _both_backwards(ops, x, c, b, w, labels, codes, relu=False):
    out = []
    for packed in (True, False):
        xt, ct, bt = _cuda(x).requires_grad_(True), _cuda(c).requires_grad_(True), _cuda(b).requires_grad_(True)
        if packed:
            y = ops.packed_codebook_linear(xt, codes, ct, bias=bt, relu=relu)
        else:
            y = ops.codebook_linear(xt, labels, ct, codes.kdim, codes.ncols, bias=bt, relu=relu)
        (y * _cuda(w)).sum().backward()                      # linear in y: both sides receive the same g
        out.append((y.detach(), xt.grad, ct.grad, bt.grad))
    return out


@pytest.mark.parametrize("m", [5, 40])
@pytest.mark.parametrize("bits,k", [(2, 4), (4, 13)])
def test_packed_codebook_linear_equals_codebook_linear_on_exact_data(env, m, bits, k):
    ops, _ = env
    x, c, lab, b, w, labels, codes = _layer_data(ops, m, m + bits, bits=bits, k=k, exact=True)
    for relu in (False, True):
        (py, px, pc, pb), (by, bx, bc, bb) = _both_backwards(ops, x, c, b, w, labels, codes, relu)
        assert torch.equal(py, by) and torch.equal(px, bx) and torch.equal(pc, bc) and torch.equal(pb, bb)
    assert np.array_equal(px.cpu().numpy(), ref.dx64(np.where(py.cpu().numpy() > 0, w, 0), lab, c, bits))


@pytest.mark.parametrize("m", [5, 40])
def test_packed_codebook_linear_gives_the_byte_centre_gradient_on_random_data(env, m):
    ops, _ = env
    x, c, lab, b, w, labels, codes = _layer_data(ops, m, m)
    (py, px, pc, pb), (by, bx, bc, bb) = _both_backwards(ops, x, c, b, w, labels, codes)
    assert torch.equal(pc, bc) and torch.equal(pb, bb)
    want, bound = ref.dx_bound(w, lab, c)
    assert np.all(np.abs(px.cpu().numpy() - want) <= bound)


@pytest.mark.parametrize("m", [5, 40])
def test_relu_masks_g_on_the_layers_own_output(env, m):
    ops, _ = env
    x, c, lab, b, w, labels, codes = _layer_data(ops, m, 100 + m)
    xt, ct = _cuda(x).requires_grad_(True), _cuda(c).requires_grad_(True)
    y = ops.packed_codebook_linear(xt, codes, ct, bias=_cuda(b), relu=True)
    gy = _cuda(w)
    y.backward(gy)
    g = torch.where(y.detach() > 0, gy, torch.zeros((), device="cuda"))
    assert bool((y.detach() == 0).any())
    assert torch.equal(xt.grad, ops.packed_codebook_matmul_dx(g, codes, ct.detach()))
    assert torch.equal(ct.grad, ops.packed_codebook_centroid_grad(_cuda(x), g, codes, dtype=torch.float32))


@pytest.mark.parametrize("m", [5, 40])
def test_no_grad_forward_is_packed_codebook_matmul(env, m):
    ops, _ = env
    x, c, lab, b, w, labels, codes = _layer_data(ops, m, 200 + m)
    xt, ct, bt = _cuda(x).requires_grad_(True), _cuda(c).requires_grad_(True), _cuda(b)
    for relu in (False, True):
        with torch.no_grad():
            assert torch.equal(ops.packed_codebook_linear(xt, codes, ct, bias=bt, relu=relu),
                               ops.packed_codebook_matmul(xt, codes, ct, bias=bt, relu=relu))
    with pytest.raises(RuntimeError, match="inference only"):
        ops.packed_codebook_matmul(xt, codes, ct)
    with pytest.raises(TypeError, match="PackedCodes"):
        ops.packed_codebook_linear(xt, labels, ct)


def test_only_the_needed_kernels_run(env, monkeypatch):
    ops, _ = env
    x, c, lab, b, w, labels, codes = _layer_data(ops, 8, 300)
    calls = []
    real_dx, real_dc = ops.packed_codebook_matmul_dx, ops.packed_codebook_centroid_grad
    monkeypatch.setattr(ops, "packed_codebook_matmul_dx", lambda *a, **k: calls.append("dx") or real_dx(*a, **k))
    monkeypatch.setattr(ops, "packed_codebook_centroid_grad", lambda *a, **k: calls.append("dc") or real_dc(*a, **k))
    for need_x, need_c, want in ((True, True, ["dx", "dc"]), (True, False, ["dx"]), (False, True, ["dc"])):
        calls.clear()
        xt, ct = _cuda(x).requires_grad_(need_x), _cuda(c).requires_grad_(need_c)
        ops.packed_codebook_linear(xt, codes, ct).sum().backward()
        assert calls == want and (xt.grad is not None) == need_x and (ct.grad is not None) == need_c
    calls.clear()
    bt = _cuda(b).requires_grad_(True)
    ops.packed_codebook_linear(_cuda(x), codes, _cuda(c), bias=bt).sum().backward()
    assert calls == [] and torch.equal(bt.grad, torch.full_like(bt, 8.0))


def test_forward_and_backward_read_nothing_back(env):
    ops, _ = env
    x, c, lab, b, w, labels, codes = _layer_data(ops, 16, 7)
    xt, ct, bt = _cuda(x).requires_grad_(True), _cuda(c).requires_grad_(True), _cuda(b).requires_grad_(True)
    gy = torch.ones(16, 150, device="cuda")
    gy40 = torch.ones(40, 150, device="cuda")
    x40 = xt[:5].detach().repeat(8, 1)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for relu in (False, True):
            ops.packed_codebook_linear(xt, codes, ct, bias=bt, relu=relu).backward(gy)
            ops.packed_codebook_linear(x40.clone().requires_grad_(True), codes, ct, relu=relu).backward(gy40)
    finally:
        torch.cuda.set_sync_debug_mode(0)


@pytest.mark.parametrize("m", [1, 16])
def test_backward_memory_is_outputs_plus_workspace(env, m):
    ops, cus = env
    kdim = ncols = 8192
    bits, k = 4, 16
    labels = torch.randint(0, k, (kdim * ncols,), device="cuda").to(torch.uint8)
    codes = ops.pack_codes(labels, kdim, ncols, k, bits)
    del labels
    ct = (torch.randn(k, device="cuda") * 0.1).requires_grad_(True)
    xt = torch.randn(m, kdim, device="cuda").requires_grad_(True)
    y = ops.packed_codebook_linear(xt, codes, ct)
    gy = torch.randn_like(y)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y.backward(gy)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    ws = ops.cbpk_dx_plan(m, kdim, ncols, bits, k, cus)["workspace"] + ops.cbpk_dc_plan(m, kdim, ncols, bits, k, cus)["workspace"]
    outputs = m * kdim * 4 + k * 4
    assert growth <= outputs + ws + (1 << 20), (growth, outputs, ws)
    assert growth < kdim * ncols                             # no byte labels (64 MiB), no W (256 MiB)


# ------------------------------------------------------------------ layers
def _model(c, labels):
    return SimpleNamespace(cluster_centers_=np.asarray(c, dtype=np.float32).reshape(-1, 1), labels_compact_=labels)


@pytest.mark.parametrize("quantized_bias", [False, True])
def test_trainable_packed_layers_match_the_inference_and_byte_trainable_ones(env, quantized_bias):
    ops, _ = env
    from neural_network_compression_amd import compressed
    from neural_network_compression_amd.neural_networks.layers import Conv2D, Dense

    rng = np.random.RandomState(31)
    torch.manual_seed(4)
    dense = Dense(784, 300, activation=torch.relu).cuda()
    conv = Conv2D(20, 50, 5, activation=torch.relu, padding="same").cuda()
    cases = ((dense, torch.randn(33, 784, device="cuda"), compressed.PackedCompressedDense, compressed.TrainablePackedCompressedDense,
              compressed.TrainableCompressedDense),
             (conv, torch.randn(3, 12, 12, 20, device="cuda"), compressed.PackedCompressedConv2D, compressed.TrainablePackedCompressedConv2D,
              compressed.TrainableCompressedConv2D))
    for layer, xin, Inf, TrPk, TrBy in cases:
        c = (rng.randn(16) * 0.1).astype(np.float32)
        wm = _model(c, _cuda(rng.randint(0, 16, size=layer.kernel.numel()).astype(np.uint8)))
        bm = None
        if quantized_bias:
            bm = _model((rng.randn(4) * 0.1).astype(np.float32), _cuda(rng.randint(0, 4, size=layer.bias.numel()).astype(np.uint8)))
        make = (lambda cls: cls.from_dense(layer, wm, bm)) if isinstance(layer, Dense) else (lambda cls: cls.from_conv(layer, wm, bm))
        inf, trpk = make(Inf), make(TrPk)
        trby = compressed._trainable(layer, wm, bm)
        assert isinstance(trby, TrBy) and isinstance(trpk, compressed._TrainableCentres)
        assert not hasattr(trpk, "labels") and trpk.packed.numel() == trpk.kdim * packed_ref.row_bytes(trpk.ncols, 4)
        with torch.no_grad():
            assert torch.equal(trpk(xin), inf(xin))
        assert torch.equal(trpk.kernel_sq_sum(), trby.kernel_sq_sum())
        assert trpk.nbytes() < trby.nbytes() and trby.nbytes() - trpk.nbytes() == trpk.kdim * trpk.ncols - trpk.packed.numel()
        assert compressed.compressed_nbytes(trpk) == trpk.nbytes()
        assert (trpk.bias_centers is not None) == quantized_bias
        # one backward through each: the centroid gradients agree bit for bit (no activation: both see the same g)
        trpk.activation = trby.activation = None
        trpk._fused_relu = trby._fused_relu = False
        for lay in (trpk, trby):
            (lay(xin) * 0.01).sum().backward()
        assert torch.equal(trpk.centers.grad, trby.centers.grad)
        if quantized_bias:
            assert torch.equal(trpk.bias_centers.grad, trby.bias_centers.grad)


class _ThreeDense(torch.nn.Module):
    def __init__(self):
        super().__init__()
        from neural_network_compression_amd.neural_networks.layers import Dense

        self.wide, self.pruned, self.narrow = Dense(64, 256, activation=torch.relu), Dense(256, 512, activation=torch.relu), Dense(512, 10)

    def get_config(self):
        return {"wide": self.wide, "pruned": self.pruned, "narrow": self.narrow}

    def forward(self, x):
        return self.narrow(self.pruned(self.wide(x)))


def test_each_trainable_form_wins_one_layer_under_the_three_way_rule(env):
    """The network of test_gpu_packed_codebook.py's forms test (a wide dense 4-bit layer, a 99 %-pruned one and a 10-column one)
    through compress_network_trainable: the same table, the trainable classes."""
    from neural_network_compression_amd import compressed

    rng = np.random.RandomState(12)
    net = _ThreeDense().cuda()
    cen = (np.arange(16) - 8).astype(np.float32) / 8.0
    models = {}
    for name, layer in net.get_config().items():
        n = layer.kernel.numel()
        lab = rng.randint(0, 16, size=n)
        if name == "pruned":
            lab = np.where(rng.rand(n) < 0.99, 8, lab)
        bl = rng.randint(0, 16, size=layer.bias.numel())
        kt, bt = _cuda(lab.astype(np.uint8)), _cuda(bl.astype(np.uint8))
        layer.set_weights([_cuda(cen[lab]).view(layer.kernel.shape), _cuda(cen[bl])])
        models[layer] = [_model(cen, kt), _model(cen, bt)]
    x = _cuda((rng.rand(9, 64) < 0.2).astype(np.float32))
    today = compressed.compress_network_trainable(net, models)
    with torch.no_grad():
        want = today(x)

    def forms(**kw):
        cnet = compressed.compress_network_trainable(net, models, **kw)
        with torch.no_grad():
            assert torch.equal(cnet(x).view(torch.int32), want.view(torch.int32)), kw      # exact data: every form, the same bits
        return [type(l).__name__ for l in cnet.get_config().values()], cnet

    B, S, P = "TrainableCompressedDense", "TrainableSparseCompressedDense", "TrainablePackedCompressedDense"
    got, cnet = forms(sparse="auto", packed="auto")
    assert got == [P, S, B]
    assert cnet.wide.nbytes() == 64 * 128 + 4 * 16 + 256 + 4 * 16 and cnet.narrow.nbytes() == 512 * 10 + 4 * 16 + 10 + 4 * 16
    assert forms(packed="auto")[0] == [P, P, B]
    assert forms(packed=True)[0] == [P, P, P]
    assert forms(sparse="auto", packed=True)[0] == [P, S, P]
    assert forms(sparse=True, packed="auto")[0] == [P, S, P]
    assert forms(sparse="auto")[0] == [B, S, B]
    got, same = forms(packed=False)
    assert got == [B, B, B] == [type(l).__name__ for l in today.get_config().values()]
    for a, b in zip(same.get_config().values(), today.get_config().values()):
        assert torch.equal(a.labels, b.labels) and torch.equal(a.centers, b.centers)
    with pytest.raises(ValueError):
        compressed.compress_network_trainable(net, models, sparse=True, packed=True)


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


def test_auto_keeps_the_byte_form_where_padded_rows_are_larger_and_17_centres_stay_bytes(env):
    from neural_network_compression_amd import compressed

    t, tr = _lenet300()
    _, test, x, _ = _data(tr, 256)
    t.quantize(test, False, 4, "linear")
    models = t.quantized_models_by_layer
    auto = compressed.compress_network_trainable(t.neural_network, models, packed="auto")
    assert type(auto.dense1) is type(auto.dense2) is compressed.TrainablePackedCompressedDense
    assert type(auto.out) is compressed.TrainableCompressedDense          # 100 x 10: 16-byte rows against 10-byte ones
    forced = compressed.compress_network_trainable(t.neural_network, models, packed=True)
    assert all(type(l) is compressed.TrainablePackedCompressedDense for l in forced.get_config().values())
    byte = compressed.compress_network_trainable(t.neural_network, models)
    assert forced.dense1.nbytes() < byte.dense1.nbytes() and forced.out.nbytes() > byte.out.nbytes()
    xb = torch.from_numpy(x).cuda()
    with torch.no_grad():
        want = t.compressed_network(packed=True)(xb)
        assert torch.equal(forced(xb), want)
    t17, _ = _lenet300(1)
    t17._prune_parameters(True)
    t17.quantize(test, True, 4, "density")
    m17 = t17.quantized_models_by_layer
    ks = {n: m17[l][0].cluster_centers_.size for n, l in t17.neural_network.get_config().items()}
    assert max(ks.values()) == 17
    net17 = compressed.compress_network_trainable(t17.neural_network, m17, packed=True)
    for n, k in ks.items():
        assert type(getattr(net17, n)) is (compressed.TrainablePackedCompressedDense if k <= 16 else compressed.TrainableCompressedDense)


def test_fine_tune_compressed_packed_lowers_the_loss_and_keeps_the_indices(env, tmp_path):
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
    acc = t.fine_tune_compressed(data, test, epochs=2, learning_rate=1e-3, packed=True)
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
    net = t.compressed_network(packed=True)
    assert all(isinstance(l, compressed.PackedCompressedDense) for l in net.get_config().values())
    t.store_compressed(str(tmp_path))
    loaded = compressed.load_network(str(tmp_path / "weights.nnc"), t.neural_network, packed=True)
    with torch.no_grad():
        assert torch.equal(net(xb[:300]), loaded(xb[:300]))


def test_lenet5_fine_tunes_its_conv_layers_with_packed_auto(env):
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
    net = compressed.compress_network_trainable(t.neural_network, models, packed="auto")
    for n in ("conv1", "conv2"):
        assert isinstance(getattr(net, n), (compressed.TrainableCompressedConv2D, compressed.TrainablePackedCompressedConv2D))
    assert any(isinstance(l, compressed._TrainablePackedCodebookLayer) for l in net.get_config().values())
    acc = t.fine_tune_compressed(data, test, epochs=1, learning_rate=1e-2, packed="auto")
    assert len(acc) == 1
    for n, c in before.items():
        after = models[getattr(t.neural_network, n)][0].cluster_centers_
        assert not np.array_equal(after, c), n
