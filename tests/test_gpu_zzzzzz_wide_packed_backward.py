"""The backward pass of the 5-, 6- and 9-bit split-plane ("wide packed") codebook layer on the GPU (csrc/nnc_cbwpgrad.hip, DESIGN.md
section 37; run with -m gpu): dx and dc against the float64 formulas (bit for bit on exact data), against the float32 bound and the
byte form's calls on random data, the padding, the autograd Function and the trainable layers widen_packed_layers builds."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_compression_amd import compressed, ops  # noqa: E402
from tests.helpers import cbgrad_ref as ref  # noqa: E402

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
WIDTHS = [(5, 17), (5, 32), (6, 33), (6, 64), (9, 257), (9, 512)]
MS, NCOLS, KDIMS = (1, 3, 16, 17, 130), (1, 127, 129, 300, 1100), (1, 33, 200)
M_SPLIT = 300   # the smallest shape class that splits m on the float32 dc tile (tests/test_wide_packed_codebook_grad_abi.py)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _case(bits, k, kdim, ncols, lo=0):
    """Made once per shape and left unchanged: labels in [lo, K) (a tenth beyond K where K < 2^bits), their codes and dyadic centres
    (multiples of 1/4 up to 4)."""
    rng = np.random.RandomState(1000 * bits + k + 7 * kdim + ncols)
    lab = rng.randint(lo, k, size=(kdim, ncols))
    if k < 1 << bits:
        lab[rng.rand(kdim, ncols) < 0.1] = (1 << bits) - 1
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    codes = ops.pack_codes_wide(_cuda(lab.astype(np.int16 if bits == 9 else np.uint8)), kdim, ncols, k)
    return codes, lab, cen


def _ints(seed, m, kdim, ncols):
    rng = np.random.RandomState(seed)
    return rng.randint(-8, 9, size=(m, kdim)).astype(np.float32), rng.randint(-8, 9, size=(m, ncols)).astype(np.float32)


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("bits,k", WIDTHS)
def test_exact_data_gives_the_float64_gradients_bit_for_bit(bits, k, dtype):
    """Centres that are multiples of 1/4 up to 4 and integer x, g up to 8: every product and partial sum of dx is exact in float32
    (at most 1100 * 8 * 16 quarter units) and in either half type, every dW is an exact integer (at most 300 * 64) binned without
    rounding, so any order gives the float64 value; a half dx and a float32 dc are that value rounded once."""
    tdt = TDT[dtype]
    for ci, (kdim, ncols) in enumerate((kd, n) for kd in KDIMS for n in NCOLS):
        codes, lab, cen = _case(bits, k, kdim, ncols)
        for m in MS + ((M_SPLIT,) if (kdim, ncols) == (200, 300) else ()):
            x, g = _ints(ci + m, m, kdim, ncols)
            xd, gd = _cuda(x).to(tdt), _cuda(g).to(tdt)
            want = torch.from_numpy(ref.dx64(g, lab, cen)).to(torch.float32)
            for out_dtype in (None, torch.float32):
                dx = ops.wide_packed_codebook_matmul_dx(gd, codes, _cuda(cen), out_dtype)
                assert dx.dtype == (tdt if out_dtype is None else torch.float32) and dx.shape == (m, kdim)
                assert torch.equal(dx.cpu(), want.to(dx.dtype)), ("dx", m, kdim, ncols, out_dtype)
            want = torch.from_numpy(ref.dc64(x, g, lab, k))
            for out in (torch.float64, torch.float32):
                dc = ops.wide_packed_codebook_centroid_grad(xd, gd, codes, dtype=out)
                assert dc.dtype == out and torch.equal(dc.cpu(), want.to(out)), ("dc", m, kdim, ncols, out)


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("bits,k", WIDTHS)
def test_random_data_is_within_the_bound_and_equals_the_byte_form(bits, k, dtype):
    """A float32 dx is within cbgrad_ref.dx_bound of the float64 product of the operands the kernel multiplies (with half g the centres
    rounded to g's dtype: those products are exact and the sums float32, so the float32 bound holds as it stands); a half dx is the
    float32 one rounded once.  dc is ops.codebook_centroid_grad on the unpacked labels bit for bit at every m and dtype (that call is
    held to section 12's bound by its own tests); above 16 rows of a half g, dx is ops.codebook_matmul_dx on them bit for bit."""
    tdt = TDT[dtype]
    for m, kdim, ncols in ((1, 33, 129), (3, 200, 300), (16, 200, 1100), (17, 33, 127), (130, 200, 300), (M_SPLIT, 200, 300), (130, 200, 1100)):
        codes, lab, _ = _case(bits, k, kdim, ncols)
        rng = np.random.RandomState(bits + m)
        cen = _cuda((0.05 * rng.standard_normal(k)).astype(np.float32))
        x, g = _cuda(rng.standard_normal((m, kdim)).astype(np.float32)).to(tdt), _cuda(rng.standard_normal((m, ncols)).astype(np.float32)).to(tdt)
        dx32 = ops.wide_packed_codebook_matmul_dx(g, codes, cen, torch.float32)
        g64, c64 = g.double().cpu().numpy(), cen.to(tdt).double().cpu().numpy()
        err, bound = np.abs(dx32.double().cpu().numpy() - ref.dx64(g64, lab, c64)), ref.dx_bound(g64, lab, c64) + 1e-30
        print(f"bits {bits} {dtype} m {m} kdim {kdim} ncols {ncols}: largest dx error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        assert torch.equal(ops.wide_packed_codebook_matmul_dx(g, codes, cen), dx32.to(tdt))
        dense = codes.to_dense()
        for out in (torch.float64, torch.float32):
            dc = ops.wide_packed_codebook_centroid_grad(x, g, codes, dtype=out)
            assert torch.isfinite(dc).all() and torch.equal(dc, ops.codebook_centroid_grad(x, g, dense, k, kdim, ncols, dtype=out)), (m, kdim, ncols, out)
        if m > 16 and dtype != "f32":
            assert torch.equal(dx32, ops.codebook_matmul_dx(g, dense, cen, kdim, ncols, out_dtype=torch.float32)), (m, kdim, ncols)


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("bits,k", [(5, 17), (6, 64), (9, 257)])
def test_no_padding_field_is_read_as_a_weight_or_binned(bits, k, dtype):
    """Centre 0 = 1e6, which rounds to Inf in fp16, and no label 0 in the matrix: the padding fields and plane bits past ncols hold
    label 0, so a padding field read as a weight gives Inf * 0 = NaN (or 1e6 * g) in dx, and one that is binned makes dc[0] non-zero."""
    tdt = TDT[dtype]
    for ncols in (1, 127, 129):
        codes, lab, cen = _case(bits, k, 33, ncols, 1)
        cen = cen.copy()
        cen[0] = 1e6
        for m in (3, 16, 130):
            x, g = _ints(m + ncols, m, 33, ncols)
            dx = ops.wide_packed_codebook_matmul_dx(_cuda(g).to(tdt), codes, _cuda(cen), torch.float32)
            assert torch.equal(dx.cpu(), torch.from_numpy(ref.dx64(g, lab, cen)).to(torch.float32)), (m, ncols)
            dc = ops.wide_packed_codebook_centroid_grad(_cuda(x).to(tdt), _cuda(g).to(tdt), codes)
            assert dc[0].item() == 0.0 and torch.equal(dc.cpu(), torch.from_numpy(ref.dc64(x, g, lab, k))), (m, ncols)


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("m", [3, 130])
@pytest.mark.parametrize("bits,k", [(5, 17), (6, 64), (9, 257)])
def test_the_linear_function_gives_the_gradients_of_the_byte_form(bits, k, m, dtype):
    """wide_packed_codebook_linear against codebook_linear on the unpacked labels, with bias and ReLU, on exact data (so both forwards
    give the same y and the same ReLU mask): the gradients of the centres and the bias bit for bit, that of x within twice the dx
    bound (each float32 value lies within the bound of the exact one) plus, for a half x, the two roundings to x's dtype."""
    tdt, (kdim, ncols) = TDT[dtype], (33, 129)
    codes, lab, cen = _case(bits, k, kdim, ncols)
    x, gy = _ints(m, m, kdim, ncols)
    bias = np.random.RandomState(m).randint(-50, 51, size=ncols).astype(np.float32)
    grads = []
    for run in (lambda xx, c, b: ops.wide_packed_codebook_linear(xx, codes, c, b, relu=True),
                lambda xx, c, b: ops.codebook_linear(xx, codes.to_dense(), c, kdim, ncols, b, relu=True)):
        leaves = [_cuda(x).to(tdt).requires_grad_(), _cuda(cen).requires_grad_(), _cuda(bias).requires_grad_()]
        y = run(*leaves)
        assert y.dtype == tdt and y.shape == (m, ncols)
        y.backward(_cuda(gy).to(tdt))
        grads.append([y.detach()] + [t.grad for t in leaves])
    (yw, dxw, dcw, dbw), (yb, dxb, dcb, dbb) = grads
    assert torch.equal(yw, yb) and (yw > 0).any() and (yw <= 0).any()
    assert dxw.dtype == tdt and dcw.dtype == dbw.dtype == torch.float32
    assert torch.equal(dcw, dcb) and torch.equal(dbw, dbb) and dcw.abs().sum() > 0
    g_eff = np.where(yw.double().cpu().numpy() > 0, gy.astype(np.float64), 0.0)
    c64 = torch.from_numpy(cen).to(tdt).double().numpy()
    eps = {"f32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}[dtype]
    tol = 2.0 * ref.dx_bound(g_eff, lab, c64) + 2.0 * eps * np.abs(ref.dx64(g_eff, lab, c64))
    assert (np.abs(dxw.double().cpu().numpy() - dxb.double().cpu().numpy()) <= tol).all()


class _Net(torch.nn.Module):
    """Conv2D 3 x 3 (3 -> 5 channels, 4 x 4 images) -> Dense 80 x 100 -> Dense 100 x 10, trainable byte layers of K = 17 centres that
    are multiples of 1/2 up to 1, integer biases: on inputs of -1, 0, 1 every activation and gradient is exact in float32 (the
    outputs stay below 2^21 eighths), whatever the order of the sums."""

    def __init__(self):
        super().__init__()
        rng = np.random.RandomState(5)
        lab = lambda n: _cuda(rng.randint(0, 17, size=n).astype(np.uint8))                       # noqa: E731
        cen, b = lambda: _cuda((rng.randint(-2, 3, size=17) / 2.0).astype(np.float32)), lambda n: _cuda(rng.randint(-2, 3, size=n).astype(np.float32))  # noqa: E731
        self.conv = compressed.TrainableCompressedConv2D(3, 3, 5, 1, lab(27 * 5), cen(), b(5), None, torch.relu)
        self.hidden = compressed.TrainableCompressedDense(80, 100, lab(8000), cen(), b(100), None, torch.relu)
        self.out = compressed.TrainableCompressedDense(100, 10, lab(1000), cen(), b(10), None, None)

    def get_config(self):
        return {"conv": self.conv, "hidden": self.hidden, "out": self.out}

    def forward(self, x):
        return self.out(self.hidden(self.conv(x).reshape(x.shape[0], -1)))


def test_widened_trainable_layers_take_the_byte_layers_step():
    net = _Net().cuda()
    assert [type(l) for l in compressed.widen_packed_layers(net).get_config().values()] == [type(l) for l in net.get_config().values()]
    wide = compressed.widen_packed_layers(net, trainable=True)
    assert [type(l).__name__ for l in wide.get_config().values()] == ["TrainableWidePackedCompressedConv2D", "TrainableWidePackedCompressedDense",
                                                                      "TrainableWidePackedCompressedDense"]
    assert type(compressed.widen_packed_layers(net, "auto", trainable=True).conv) is compressed.TrainableCompressedConv2D
    assert net.hidden.nbytes() - wide.hidden.nbytes() == 80 * (100 - 80)   # a row of 100 labels: 64 bytes of fields, 16 of plane
    packed = {n: l.packed.clone() for n, l in wide.get_config().items()}
    rng = np.random.RandomState(9)
    x, w = _cuda(rng.randint(-1, 2, size=(6, 4, 4, 3)).astype(np.float32)), _cuda(rng.choice([-1.0, 1.0], size=(6, 10)).astype(np.float32))
    for model in (net, wide):
        opt = torch.optim.SGD(model.parameters(), lr=2.0 ** -10)
        y = model(x)
        (y * w).sum().backward()
        model.y = y.detach()
        model.grads = {n: l.centers.grad.clone() for n, l in model.get_config().items()}
        opt.step()
    assert torch.equal(net.y, wide.y)
    for name, layer in wide.get_config().items():
        byte = getattr(net, name)
        assert torch.equal(wide.grads[name], net.grads[name]) and net.grads[name].abs().sum() > 0, name
        assert torch.equal(layer.centers, byte.centers) and torch.equal(layer.counts, byte.counts), name
        assert torch.equal(layer.packed, packed[name]) and not hasattr(layer, "labels"), name
