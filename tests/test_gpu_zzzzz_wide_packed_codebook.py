"""The 5-, 6- and 9-bit split-plane ("wide packed") codebook layer on the GPU (csrc/nnc_cbwp.hip; run with
-m gpu): the pack against a NumPy statement of the layout, the product against the float64 product (bit for bit on exact data, within
the float32 bound on random data) and the layers that widen_packed_layers builds."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_compression_amd import compressed, ops  # noqa: E402

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
WIDTHS = [(5, 17), (5, 32), (6, 33), (6, 64), (9, 257), (9, 512)]
MS, NCOLS, KDIMS, KDIM_SPLIT = (1, 3, 16, 17, 130), (1, 127, 129, 300), (1, 33, 200), 2048


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _labels(lab, dtype):
    """the labels on the device one element into their storage"""
    buf = torch.zeros(lab.size + 1, dtype=dtype, device="cuda")
    buf[1:] = _cuda(lab.ravel().astype(np.int16 if dtype is torch.int16 else np.uint8))
    return buf[1:]


def _layout(lab, bits):
    """the form of include/nnc_cbwp.h in NumPy: per row the base part, then the planes, each padded with zeros to 16 bytes"""
    base, (kdim, ncols) = (8 if bits == 9 else 4), lab.shape
    bb, pb = 16 * -(-ncols * base // 128), 16 * -(-ncols // 128)
    rows = np.zeros((kdim, bb + (bits - base) * pb), dtype=np.uint8)
    if base == 8:
        rows[:, :ncols] = lab & 255
    else:
        lo = np.zeros((kdim, ncols + ncols % 2), dtype=np.uint8)
        lo[:, :ncols] = lab & 15
        rows[:, :lo.shape[1] // 2] = lo[:, 0::2] | lo[:, 1::2] << 4
    for p in range(bits - base):
        plane = np.packbits((lab >> (base + p)) & 1, axis=1, bitorder="little")
        rows[:, bb + p * pb: bb + p * pb + plane.shape[1]] = plane
    return rows


@pytest.mark.parametrize("k,ldt", [(17, torch.uint8), (64, torch.uint8), (257, torch.uint8), (33, torch.int16), (512, torch.int16)])
def test_pack_is_the_layout_and_unpack_returns_the_labels(k, ldt):
    bits = ops.wide_packed_bits(k)
    for kdim in (1, 33):
        for ncols in NCOLS:
            lab = np.random.RandomState(k + kdim + ncols).randint(0, min(k, 256 if ldt is torch.uint8 else k), size=(kdim, ncols))
            lab[-1, -1] = min(k, 256 if ldt is torch.uint8 else 1 << bits) - 1
            dev = _labels(lab, ldt)
            codes = ops.pack_codes_wide(dev, kdim, ncols, k)
            assert codes.bits == bits and codes.nbytes == ops.wide_packed_nbytes(kdim, ncols, bits) and codes.packed.data_ptr() % 256 == 0
            assert np.array_equal(codes.packed.cpu().numpy().reshape(kdim, -1), _layout(lab, bits)), (kdim, ncols)   # the padding is 0
            back = codes.to_dense()
            assert back.dtype == (torch.int16 if bits == 9 else torch.uint8) and np.array_equal(back.cpu().numpy().reshape(kdim, ncols), lab)
    if ldt is torch.int16 or bits < 8:
        lab[0, 0] = 1 << bits
        with pytest.raises(ValueError, match="do not fit"):
            ops.pack_codes_wide(_labels(lab, ldt), kdim, ncols, k)


@functools.lru_cache(maxsize=None)
def _exact_case(bits, k, kdim, ncols):
    """Made once per shape and left unchanged: labels (a tenth beyond K where K < 2^bits), their codes, dyadic centres, an integer
    bias and the float64 W (0 where the label is beyond K)."""
    rng = np.random.RandomState(1000 * bits + k + 7 * kdim + ncols)
    lab = rng.randint(0, k, size=(kdim, ncols))
    if k < 1 << bits:
        lab[rng.rand(kdim, ncols) < 0.1] = (1 << bits) - 1
    cen = (rng.randint(-16, 17, size=k) / 4.0).astype(np.float32)
    w = np.where(lab < k, cen.astype(np.float64)[np.minimum(lab, k - 1)], 0.0)
    codes = ops.pack_codes_wide(_labels(lab, torch.int16 if bits == 9 else torch.uint8), kdim, ncols, k)
    return codes, _cuda(cen), w, rng.randint(-50, 51, size=ncols).astype(np.float32)


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("bits,k", WIDTHS)
def test_exact_data_gives_the_float64_product_bit_for_bit(bits, k, dtype):
    """Centres that are multiples of 1/4 up to 4 and integer x up to 8: every product and partial sum is exact in float32 (at most
    2048 * 32 * 4 quarter units < 2^24) and in either half type, so any summation order gives the float64 product; a half result is
    that value rounded once."""
    tdt, cus = TDT[dtype], ops.device_info()[1]
    ms = MS if dtype == "f32" else (1, 3, 16, 17, 130)
    assert all(ops.cbwp_plan(tdt, m, KDIM_SPLIT, n, bits, k, cus)["splits"] > 1 for m in ms for n in NCOLS)
    assert {ops.cbwp_plan(tdt, m, 33, 129, bits, k, cus)["path"] for m in ms} == {1, 2 if dtype == "f32" else 5}
    for ci, (kdim, ncols) in enumerate((kd, n) for kd in KDIMS + (KDIM_SPLIT,) for n in NCOLS):
        codes, cen, w, bias = _exact_case(bits, k, kdim, ncols)
        for m in ms:
            x = np.random.RandomState(ci + m).randint(-8, 9, size=(m, kdim)).astype(np.float32)
            use_bias, relu = (ci + m) % 2 == 0, (ci + m) % 3 == 0
            want = x.astype(np.float64) @ w + (bias if use_bias else 0.0)
            want = torch.from_numpy(np.maximum(want, 0.0) if relu else want)
            for out_dtype in (None, torch.float32):
                y = ops.wide_packed_codebook_matmul(_cuda(x).to(tdt), codes, cen, _cuda(bias) if use_bias else None, relu, out_dtype)
                assert y.dtype == (tdt if out_dtype is None else torch.float32) and y.shape == (m, ncols)
                assert torch.equal(y.cpu(), want.to(torch.float32).to(y.dtype)), (m, kdim, ncols, out_dtype)


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("bits,k", [(5, 17), (6, 64), (9, 257)])
def test_random_data_is_within_the_float32_bound(bits, k, dtype):
    """float32 output: within 2 kdim 2^-24 (|x| |W| + |b|) of the float64 product of the operands the kernel multiplies (with half x
    the centres rounded to x's dtype: those products are exact and the sums float32, so the float32 bound holds for them as it
    stands).  Half output: the float32 output rounded once, which is what tests/test_gpu_packed_codebook_h16.py holds the packed form
    to."""
    tdt = TDT[dtype]
    for m, kdim, ncols in ((3, 200, 300), (16, KDIM_SPLIT, 129), (17, 33, 127), (130, KDIM_SPLIT, 300)):
        rng = np.random.RandomState(bits + m)
        lab, cen = rng.randint(0, k, size=(kdim, ncols)), (0.05 * rng.standard_normal(k)).astype(np.float32)
        x, bias = _cuda(rng.standard_normal((m, kdim)).astype(np.float32)).to(tdt), rng.standard_normal(ncols).astype(np.float32)
        codes = ops.pack_codes_wide(_labels(lab, torch.int16), kdim, ncols, k)
        w64 = torch.from_numpy(cen).to(tdt).double().numpy()[lab]
        x64 = x.double().cpu().numpy()
        y32 = ops.wide_packed_codebook_matmul(x, codes, _cuda(cen), _cuda(bias), out_dtype=torch.float32)
        err = np.abs(y32.double().cpu().numpy() - (x64 @ w64 + bias))
        bound = 2.0 * kdim * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64) + np.abs(bias)) + 1e-30
        print(f"bits {bits} {dtype} m {m} kdim {kdim} ncols {ncols}: largest error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        assert torch.equal(ops.wide_packed_codebook_matmul(x, codes, _cuda(cen), _cuda(bias)), y32.to(tdt))


class _Net(torch.nn.Module):
    """Conv2D 3 x 3 (3 -> 5 channels, 4 x 4 images) -> Dense 80 x 100 -> Dense 100 x 10, every layer with K = 17 centres"""

    def __init__(self):
        super().__init__()
        rng = np.random.RandomState(5)
        lab = lambda n: _cuda(rng.randint(0, 17, size=n).astype(np.uint8))                       # noqa: E731
        cen, b = lambda: _cuda((0.2 * rng.standard_normal(17)).astype(np.float32)), lambda n: _cuda(rng.standard_normal(n).astype(np.float32))  # noqa: E731
        self.conv = compressed.CompressedConv2D.from_codes(3, 3, 5, 1, lab(27 * 5), cen(), b(5), torch.relu)
        self.hidden = compressed.CompressedDense(80, 100, lab(8000), cen(), b(100), torch.relu)
        self.out = compressed.CompressedDense(100, 10, lab(1000), cen(), b(10), None)

    def get_config(self):
        return {"conv": self.conv, "hidden": self.hidden, "out": self.out}

    def forward(self, x):
        return self.out(self.hidden(self.conv(x).reshape(x.shape[0], -1)))


def test_widened_layers_compute_what_the_byte_layers_compute():
    """Every layer of the widened network, on the input it meets there, is within the float32 bound of the float64 product with the
    byte layer's weights, as the byte layer is; "auto" keeps the layers whose 16-byte parts outweigh a byte per weight."""
    net = _Net().cuda()
    wide, auto = compressed.widen_packed_layers(net), compressed.widen_packed_layers(net, "auto")
    assert [type(l).__name__ for l in wide.get_config().values()] == ["WidePackedCompressedConv2D", "WidePackedCompressedDense", "WidePackedCompressedDense"]
    assert [type(l) for l in auto.get_config().values()] == [compressed.CompressedConv2D, compressed.WidePackedCompressedDense, compressed.CompressedDense]
    row = lambda n: 16 * -(-n * 4 // 128) + 16 * -(-n // 128)                                    # noqa: E731
    assert compressed.compressed_nbytes(net) - compressed.compressed_nbytes(auto) == 80 * (100 - row(100)) > 0
    assert compressed.compressed_nbytes(net) - compressed.compressed_nbytes(wide) == 27 * (5 - row(5)) + 80 * (100 - row(100)) + 100 * (10 - row(10))
    with pytest.raises(ValueError):
        compressed.widen_packed_layers(net, "yes")
    seen = {}
    for name, layer in wide.get_config().items():
        layer.register_forward_hook(lambda mod, inp, out, name=name: seen.__setitem__(name, (inp[0], out)))
    x = torch.randn(6, 4, 4, 3, device="cuda")
    with torch.no_grad():
        y = wide(x)
    assert y.shape == (6, 10) and torch.isfinite(y).all()
    for name, byte in net.get_config().items():
        xin, got = seen[name]
        if name == "conv":
            xin = compressed.conv_patches(xin, 3, 1).reshape(-1, 27)
        x64, b64 = xin.double().cpu().numpy(), byte.bias.double().cpu().numpy()
        w64 = byte.centers.double().cpu().numpy()[byte.labels.cpu().numpy().astype(np.int64)].reshape(byte.kdim, byte.ncols)
        want = x64 @ w64 + b64
        bound = 2.0 * byte.kdim * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64) + np.abs(b64)) + 1e-30
        want = np.maximum(want, 0.0) if byte.activation is torch.relu else want
        assert (np.abs(got.double().cpu().numpy().reshape(want.shape) - want) <= bound).all(), name
        with torch.no_grad():
            assert (np.abs(byte(seen[name][0]).double().cpu().numpy().reshape(want.shape) - want) <= bound).all(), name
