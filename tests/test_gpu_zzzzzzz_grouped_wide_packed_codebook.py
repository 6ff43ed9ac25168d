"""The group-wise codebook layer on 5- and 6-bit split-plane indices on the GPU (csrc/nnc_cbwp_grouped.hip; run
with -m gpu): the product against the float64 product (bit for bit on exact data, within the float32 bound on random data), against
the ungrouped call with one group and against the group-wise byte form on the MFMA tile, and the layers widen_grouped_layers builds."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_compression_amd import compressed, ops  # noqa: E402

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
WIDTHS = [(5, 17), (5, 32), (6, 33), (6, 64)]
MS, NCOLS, KDIMS, KDIM_SPLIT, GROUP_ROWS = (1, 3, 16, 17, 130), (1, 127, 129, 300), (1, 33, 200), 2048, (32, 96)
STREAM, TILED, MFMA = 1, 2, 5


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _weights(lab, cen, rows):
    """float64 W[i, o] = cen[i // rows][lab[i, o]], 0 where the label is beyond K"""
    k = cen.shape[1]
    group = np.arange(lab.shape[0])[:, None] // rows
    return np.where(lab < k, cen.astype(np.float64)[group, np.minimum(lab, k - 1)], 0.0)


@functools.lru_cache(maxsize=None)
def _exact_case(bits, k, kdim, ncols, rows):
    """Made once per shape and left unchanged: labels (a tenth beyond K where K < 2^bits), their codes, per group a draw of its own
    of multiples of 1/4 in [-4, 4] (distinct while K <= 33, the number of such values), an integer bias and the float64 W."""
    rng = np.random.RandomState(1000 * bits + k + 7 * kdim + ncols + rows)
    lab = rng.randint(0, k, size=(kdim, ncols))
    if k < 1 << bits:
        lab[rng.rand(kdim, ncols) < 0.1] = (1 << bits) - 1
    groups = -(-kdim // rows)
    cen = np.stack([rng.choice(np.arange(-16, 17), size=k, replace=k > 33) / 4.0 for _ in range(groups)]).astype(np.float32)
    codes = ops.pack_codes_wide(_cuda(lab.astype(np.uint8)), kdim, ncols, k)
    return codes, _cuda(cen), _weights(lab, cen, rows), rng.randint(-50, 51, size=ncols).astype(np.float32)


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("bits,k", WIDTHS)
def test_exact_data_gives_the_float64_product_bit_for_bit(bits, k, dtype):
    """Centres that are multiples of 1/4 up to 4 and integer x up to 8: every product and partial sum is exact in float32 (at most
    2048 * 32 * 4 quarter units < 2^24) and in either half type, so any summation order gives the float64 product; a half result is
    that value rounded once.  group_rows = 96 divides neither 200 nor 2048: boundaries inside batches, TB_K steps and splits."""
    tdt, cus = TDT[dtype], ops.device_info()[1]
    assert all(ops.cbwp_grouped_plan(tdt, m, KDIM_SPLIT, n, bits, k, 96, cus)["splits"] > 1 for m in MS for n in NCOLS)
    assert {ops.cbwp_grouped_plan(tdt, m, 33, 129, bits, k, 32, cus)["path"] for m in MS} == {STREAM, TILED if dtype == "f32" else MFMA}
    for ci, (kdim, ncols, rows) in enumerate((kd, n, g) for kd in KDIMS + (KDIM_SPLIT,) for n in NCOLS for g in GROUP_ROWS):
        codes, cen, w, bias = _exact_case(bits, k, kdim, ncols, rows)
        for m in MS:
            x = np.random.RandomState(ci + m).randint(-8, 9, size=(m, kdim)).astype(np.float32)
            use_bias, relu = (ci + m) % 2 == 0, (ci + m) % 3 == 0
            want = x.astype(np.float64) @ w + (bias if use_bias else 0.0)
            want = torch.from_numpy(np.maximum(want, 0.0) if relu else want)
            for out_dtype in (None, torch.float32):
                y = ops.grouped_wide_packed_codebook_matmul(_cuda(x).to(tdt), codes, cen, rows, _cuda(bias) if use_bias else None, relu, out_dtype)
                assert y.dtype == (tdt if out_dtype is None else torch.float32) and y.shape == (m, ncols)
                assert torch.equal(y.cpu(), want.to(torch.float32).to(y.dtype)), (m, kdim, ncols, rows, out_dtype)


def _random_case(bits, k, m, kdim, ncols, rows, tdt, seed):
    rng = np.random.RandomState(seed)
    lab = rng.randint(0, k, size=(kdim, ncols))
    cen = (0.05 * rng.standard_normal((-(-kdim // rows), k))).astype(np.float32)
    x = _cuda(rng.standard_normal((m, kdim)).astype(np.float32)).to(tdt)
    return lab, cen, x, rng.standard_normal(ncols).astype(np.float32)


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("bits,k", [(5, 17), (6, 64)])
def test_one_group_is_the_ungrouped_call(bits, k, dtype):
    """group_rows >= kdim on random float data: the bits of ops.wide_packed_codebook_matmul on the stream, tiled and MFMA paths."""
    for m in (3, 17, 130):
        for kdim, ncols in ((200, 300), (KDIM_SPLIT, 129)):
            lab, cen, x, bias = _random_case(bits, k, m, kdim, ncols, KDIM_SPLIT, TDT[dtype], bits + m)
            codes = ops.pack_codes_wide(_cuda(lab.astype(np.uint8)), kdim, ncols, k)
            got = ops.grouped_wide_packed_codebook_matmul(x, codes, _cuda(cen), KDIM_SPLIT, _cuda(bias), True)
            want = ops.wide_packed_codebook_matmul(x, codes, _cuda(cen[0]), _cuda(bias), True)
            assert got.dtype == want.dtype and torch.equal(got.view(torch.int16).cpu(), want.view(torch.int16).cpu()), (m, kdim, ncols)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("bits,k", [(5, 17), (6, 64)])
def test_mfma_tile_gives_the_byte_grouped_forms_bits(bits, k, dtype):
    """Random centres and x: the bits of ops.grouped_codebook_matmul on the unpacked labels.  Centre 0 of the last group is NaN and no
    label of that group is 0: only the padding past ncols and the rows of the last k step past kdim hold label 0 there, and neither
    may reach an output."""
    for m in (17, 130):
        for rows in GROUP_ROWS:
            for kdim, ncols in ((200, 300), (KDIM_SPLIT, 129)):
                lab, cen, x, bias = _random_case(bits, k, m, kdim, ncols, rows, TDT[dtype], bits + m + rows)
                last = (kdim - 1) // rows
                lab[last * rows:] = np.maximum(lab[last * rows:], 1)
                cen[last, 0] = np.nan
                codes = ops.pack_codes_wide(_cuda(lab.astype(np.uint8)), kdim, ncols, k)
                for out_dtype in (None, torch.float32):
                    got = ops.grouped_wide_packed_codebook_matmul(x, codes, _cuda(cen), rows, _cuda(bias), False, out_dtype)
                    want = ops.grouped_codebook_matmul(x, codes.to_dense(), _cuda(cen), kdim, ncols, rows, _cuda(bias), False, out_dtype)
                    assert torch.isfinite(got).all() and got.dtype == want.dtype and torch.equal(got.cpu(), want.cpu()), (m, rows, kdim, ncols)


@pytest.mark.parametrize("bits,k", [(5, 17), (6, 64)])
def test_random_float32_data_is_within_the_float32_bound(bits, k):
    """Within 2 kdim 2^-24 (|x| |W| + |b|) of the float64 product of the operands the kernel multiplies (section 36's bound), on the
    stream path, on the tiled path and through the split-K combine, with group boundaries off every batch, step and split."""
    for m, kdim, ncols in ((3, 200, 300), (16, KDIM_SPLIT, 129), (130, KDIM_SPLIT, 300)):
        lab, cen, x, bias = _random_case(bits, k, m, kdim, ncols, 96, torch.float32, bits + m)
        codes = ops.pack_codes_wide(_cuda(lab.astype(np.uint8)), kdim, ncols, k)
        w64, x64 = _weights(lab, cen, 96), x.double().cpu().numpy()
        y = ops.grouped_wide_packed_codebook_matmul(x, codes, _cuda(cen), 96, _cuda(bias))
        err = np.abs(y.double().cpu().numpy() - (x64 @ w64 + bias))
        bound = 2.0 * kdim * 2.0 ** -24 * (np.abs(x64) @ np.abs(w64) + np.abs(bias)) + 1e-30
        print(f"bits {bits} m {m} kdim {kdim} ncols {ncols}: largest error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()


class _Net(torch.nn.Module):
    """Grouped Dense layers on exact data (centres multiples of 1/4, integer bias): 96 x 300 with K = 17 and 100 x 10 with K = 33, and
    two 64 x 8 layers of K = 16 and K = 65, which the split-plane form does not take."""

    def __init__(self, seed=5):
        super().__init__()
        rng = np.random.RandomState(seed)
        for name, kdim, ncols, k in (("wide", 96, 300, 17), ("small", 100, 10, 33), ("k16", 64, 8, 16), ("k65", 64, 8, 65)):
            cen = _cuda((rng.randint(-16, 17, size=(-(-kdim // 32), k)) / 4.0).astype(np.float32))
            layer = compressed.GroupedCompressedDense(kdim, ncols, 32, _cuda(rng.randint(0, k, size=kdim * ncols).astype(np.uint8)), cen,
                                                      _cuda(rng.randint(-9, 10, size=ncols).astype(np.float32)), torch.relu)
            setattr(self, name, layer)

    def get_config(self):
        return {"wide": self.wide, "small": self.small, "k16": self.k16, "k65": self.k65}


def test_widen_grouped_layers():
    net = _Net().cuda()
    wide, auto = compressed.widen_grouped_layers(net), compressed.widen_grouped_layers(net, "auto")
    G, W = compressed.GroupedCompressedDense, compressed.GroupedWidePackedCompressedDense
    assert [type(l) for l in wide.get_config().values()] == [W, W, G, G] and [type(l) for l in auto.get_config().values()] == [W, G, G, G]
    row = lambda n, planes: 16 * -(-n * 4 // 128) + planes * 16 * -(-n // 128)                   # noqa: E731
    assert compressed.compressed_nbytes(net) - compressed.compressed_nbytes(auto) == 96 * (300 - row(300, 1)) > 0
    assert compressed.compressed_nbytes(net) - compressed.compressed_nbytes(wide) == 96 * (300 - row(300, 1)) + 100 * (10 - row(10, 2))
    with pytest.raises(ValueError):
        compressed.widen_grouped_layers(net, "yes")
    other = compressed.widen_grouped_layers(_Net(6).cuda())
    for name in ("wide", "small"):
        byte, made, second = getattr(net, name), getattr(wide, name), getattr(other, name)
        assert list(made.state_dict().keys()) == ["packed", "centers", "bias"] and not list(made.parameters())
        for tdt in TDT.values():
            x = torch.randint(-8, 9, (19, byte.kdim), device="cuda").to(tdt)
            with torch.no_grad():
                got, want = made(x), byte(x)
                assert got.dtype == tdt and torch.equal(got.cpu(), want.cpu()), (name, tdt)
        with torch.no_grad():
            result = made.load_state_dict(second.state_dict())
            assert not result.missing_keys and not result.unexpected_keys
            assert not torch.equal(made(x), want) and torch.equal(made(x), second(x))
