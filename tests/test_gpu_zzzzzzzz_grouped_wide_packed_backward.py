"""The backward pass of the group-wise codebook layer on 5- and 6-bit split-plane indices on the GPU (csrc/nnc_cbwpgrad_grouped.hip,
DESIGN.md section 39; run with -m gpu): dx and dc against the float64 formulas taken group by group (bit for bit on exact data),
against the float32 bound and the group-wise byte form's calls on random data, the padding, the autograd Function and the trainable
layers widen_grouped_layers builds."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_compression_amd import _native as nat  # noqa: E402
from neural_network_compression_amd import compressed, ops  # noqa: E402
from tests.helpers import grouped_grad_ref as ref  # noqa: E402

TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
WIDTHS = [(5, 17), (5, 32), (6, 33), (6, 64)]
MS, NCOLS, KDIMS, GROUP_ROWS = (1, 3, 16, 17, 130), (1, 127, 129, 300, 1100), (1, 33, 200), (32, 96)
M_SPLIT = 300   # splits m on the float32 dc tile at (200, 300), as in tests/test_gpu_zzzzzz_wide_packed_backward.py


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _shape(m, kdim, ncols, k, group_rows):
    return dict(m=m, kdim=kdim, ncols=ncols, k=k, group_rows=group_rows, off=0)


@functools.lru_cache(maxsize=None)
def _case(bits, k, kdim, ncols, group_rows, lo=0):
    """Made once per shape and left unchanged: labels in [lo, K) (a tenth beyond K where K < 2^bits), their codes and dyadic centres
    (multiples of 1/4 up to 4), drawn per group."""
    rng = np.random.RandomState(1000 * bits + k + 7 * kdim + ncols + group_rows)
    lab = rng.randint(lo, k, size=(kdim, ncols))
    if k < 1 << bits:
        lab[rng.rand(kdim, ncols) < 0.1] = (1 << bits) - 1
    cen = (rng.randint(-16, 17, size=(max(1, -(-kdim // group_rows)), k)) / 4.0).astype(np.float32)
    return ops.pack_codes_wide(_cuda(lab.astype(np.uint8)), kdim, ncols, k), lab, cen


@functools.lru_cache(maxsize=None)
def _exact(bits, k, kdim, ncols, group_rows, m, lo=0):
    """Integer x and g up to 8 and the float64 gradients of the case, shared by the three dtypes."""
    _, lab, cen = _case(bits, k, kdim, ncols, group_rows, lo)
    rng = np.random.RandomState(m + kdim + ncols)
    x, g = rng.randint(-8, 9, size=(m, kdim)).astype(np.float32), rng.randint(-8, 9, size=(m, ncols)).astype(np.float32)
    c = _shape(m, kdim, ncols, k, group_rows)
    return x, g, torch.from_numpy(ref.dx64(c, g, lab, cen)), torch.from_numpy(ref.dc64(c, x, g, lab))


def test_the_shapes_reach_every_path_and_walk():
    """From the plans at 256 CUs: the shapes below run the stream, the float32 tile and the MFMA kernels of both directions, split
    ncols and m, and put four groups into one workgroup's tile."""
    f32, bf16 = torch.float32, torch.bfloat16
    for bits, k in WIDTHS:
        dxp = lambda dt, m, n, r: ops.cbwp_grouped_dx_plan(dt, m, 200, n, bits, k, r, 256)       # noqa: E731
        dcp = lambda dt, m, n, r: ops.cbwp_grouped_dc_plan(dt, m, 200, n, bits, k, r, 256)       # noqa: E731
        assert dxp(f32, 16, 1100, 32)["path"] == dcp(f32, 16, 1100, 32)["path"] == nat.CBMM_STREAM and dxp(f32, 16, 1100, 32)["splits"] >= 2
        assert dcp(f32, 16, 1100, 32)["max_groups_per_workgroup"] >= 2
        assert dxp(f32, 130, 300, 32)["path"] == nat.CBMM_TILED and dxp(f32, 130, 300, 32)["splits"] >= 2
        assert dxp(bf16, 130, 300, 96)["path"] == dcp(bf16, 130, 300, 96)["path"] == nat.CBMM_MFMA and dcp(bf16, 130, 300, 96)["splits"] >= 2
        p = dcp(f32, M_SPLIT, 300, 32)
        assert p["path"] == nat.CBMM_TILED and p["splits"] > 1 and dcp(f32, 130, 300, 32)["splits"] == 1
        assert p["max_groups_per_workgroup"] >= 3 and p["held"] == 4 and dxp(bf16, 130, 300, 32)["max_groups_per_workgroup"] >= 3
        assert dxp(f32, 130, 300, 96)["held"] == 2 and dxp(f32, 130, 300, 96)["groups"] == 3


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("bits,k", WIDTHS)
def test_exact_data_gives_the_float64_gradients_bit_for_bit(bits, k, dtype):
    """Centres that are multiples of 1/4 up to 4 (drawn per group) and integer x, g up to 8: every product and partial sum of dx is
    exact in float32 (at most 1100 * 8 * 16 quarter units) and in either half type, every dW is an exact integer (at most 300 * 64)
    binned without rounding, so any order gives the float64 value of the group-wise formulas; a half dx and a float32 dc are that
    value rounded once.  kdim 1, 33 and 200 at group_rows 32 and 96: a group of one row, a short last group, four groups in a tile."""
    tdt = TDT[dtype]
    for kdim, ncols, group_rows in ((kd, n, r) for kd in KDIMS for n in NCOLS for r in GROUP_ROWS):
        codes, _, cen = _case(bits, k, kdim, ncols, group_rows)
        for m in MS + ((M_SPLIT,) if (kdim, ncols) == (200, 300) else ()):
            x, g, dx64, dc64 = _exact(bits, k, kdim, ncols, group_rows, m)
            xd, gd = _cuda(x).to(tdt), _cuda(g).to(tdt)
            for out_dtype in (None, torch.float32):
                dx = ops.grouped_wide_packed_codebook_matmul_dx(gd, codes, _cuda(cen), group_rows, out_dtype)
                assert dx.dtype == (tdt if out_dtype is None else torch.float32) and dx.shape == (m, kdim)
                assert torch.equal(dx.cpu(), dx64.to(torch.float32).to(dx.dtype)), ("dx", m, kdim, ncols, group_rows, out_dtype)
            for out in (torch.float64, torch.float32):
                dc = ops.grouped_wide_packed_codebook_centroid_grad(xd, gd, codes, group_rows, dtype=out)
                assert dc.dtype == out and torch.equal(dc.cpu(), dc64.to(out)), ("dc", m, kdim, ncols, group_rows, out)


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("bits,k", WIDTHS)
def test_random_data_is_within_the_bound_and_equals_the_byte_form(bits, k, dtype):
    """A float32 dx is within grouped_grad_ref.dx_bound of the float64 product of the operands the kernel multiplies (with half g the
    centres rounded to g's dtype: those products are exact and the sums float32, so the float32 bound holds as it stands); a half dx is
    the float32 one rounded once.  dc is ops.grouped_codebook_centroid_grad on the unpacked labels bit for bit at every m and dtype;
    above 16 rows of a half g, dx is ops.grouped_codebook_matmul_dx on them bit for bit.  With one group (group_rows >= kdim) dx and dc
    are the ungrouped wide_packed_* calls bit for bit."""
    tdt = TDT[dtype]
    for m, kdim, ncols, group_rows in ((1, 33, 129, 32), (3, 200, 300, 96), (16, 200, 1100, 32), (17, 33, 127, 32), (130, 200, 300, 32),
                                       (M_SPLIT, 200, 300, 96), (130, 200, 1100, 96), (16, 200, 300, 224), (130, 200, 300, 256)):
        codes, lab, _ = _case(bits, k, kdim, ncols, group_rows)
        rng = np.random.RandomState(bits + m)
        groups = max(1, -(-kdim // group_rows))
        cen = _cuda((0.05 * rng.standard_normal((groups, k))).astype(np.float32))
        x, g = _cuda(rng.standard_normal((m, kdim)).astype(np.float32)).to(tdt), _cuda(rng.standard_normal((m, ncols)).astype(np.float32)).to(tdt)
        dx32 = ops.grouped_wide_packed_codebook_matmul_dx(g, codes, cen, group_rows, torch.float32)
        c, g64, c64 = _shape(m, kdim, ncols, k, group_rows), g.double().cpu().numpy(), cen.to(tdt).double().cpu().numpy()
        err, bound = np.abs(dx32.double().cpu().numpy() - ref.dx64(c, g64, lab, c64)), ref.dx_bound(c, g64, lab, c64) + 1e-30
        print(f"bits {bits} {dtype} m {m} kdim {kdim} ncols {ncols} group_rows {group_rows}: largest dx error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        assert torch.equal(ops.grouped_wide_packed_codebook_matmul_dx(g, codes, cen, group_rows), dx32.to(tdt))
        dense = codes.to_dense()
        dcs = {out: ops.grouped_wide_packed_codebook_centroid_grad(x, g, codes, group_rows, dtype=out) for out in (torch.float64, torch.float32)}
        for out, dc in dcs.items():
            want = ops.grouped_codebook_centroid_grad(x, g, dense, k, kdim, ncols, group_rows, dtype=out)
            assert torch.isfinite(dc).all() and torch.equal(dc, want), (m, kdim, ncols, group_rows, out)
        if m > 16 and dtype != "f32":
            assert torch.equal(dx32, ops.grouped_codebook_matmul_dx(g, dense, cen, kdim, ncols, group_rows, out_dtype=torch.float32)), (m, kdim, ncols)
        if groups == 1:
            assert torch.equal(dx32, ops.wide_packed_codebook_matmul_dx(g, codes, cen[0], torch.float32)), (m, group_rows)
            assert torch.equal(dcs[torch.float64][0], ops.wide_packed_codebook_centroid_grad(x, g, codes)), (m, group_rows)


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("bits,k", WIDTHS)
def test_no_padding_field_is_read_as_a_weight_or_binned(bits, k, dtype):
    """Centre 0 of every group = 1e6, which rounds to Inf in fp16, and no label 0 in the matrix: the padding fields and plane bits past
    ncols hold label 0, so a padding field read as a weight gives Inf * 0 = NaN (or 1e6 * g) in dx, and one that is binned makes
    dc[:, 0] non-zero.  The tenth of the labels that are >= k (k < 2^bits) contribute nothing: the references leave them out."""
    tdt = TDT[dtype]
    for ncols in (1, 127, 129):
        codes, _, cen = _case(bits, k, 33, ncols, 32, 1)
        cen = cen.copy()
        cen[:, 0] = 1e6
        for m in (3, 16, 130):
            x, g, dx64, dc64 = _exact(bits, k, 33, ncols, 32, m, 1)   # (no label reads centre 0: dx64 does not depend on it)
            dx = ops.grouped_wide_packed_codebook_matmul_dx(_cuda(g).to(tdt), codes, _cuda(cen), 32, torch.float32)
            assert torch.equal(dx.cpu(), dx64.to(torch.float32)), (m, ncols)
            dc = ops.grouped_wide_packed_codebook_centroid_grad(_cuda(x).to(tdt), _cuda(g).to(tdt), codes, 32)
            assert (dc[:, 0] == 0).all() and torch.equal(dc.cpu(), dc64), (m, ncols)


@pytest.mark.parametrize("dtype", list(TDT))
@pytest.mark.parametrize("m", [3, 130])
@pytest.mark.parametrize("bits,k", WIDTHS)
def test_the_linear_function_gives_the_gradients_of_the_byte_form(bits, k, m, dtype):
    """grouped_wide_packed_codebook_linear against grouped_codebook_linear on the unpacked labels, with bias and ReLU, on exact data
    (so both forwards give the same y and the same ReLU mask): the gradients of the centres and the bias bit for bit, that of x within
    twice the dx bound (each float32 value lies within the bound of the exact one) plus, for a half x, the two roundings to x's dtype."""
    tdt, (kdim, ncols, group_rows) = TDT[dtype], (200, 129, 96)
    codes, lab, cen = _case(bits, k, kdim, ncols, group_rows)
    x, gy = _exact(bits, k, kdim, ncols, group_rows, m)[:2]
    bias = np.random.RandomState(m).randint(-50, 51, size=ncols).astype(np.float32)
    grads = []
    for run in (lambda xx, c, b: ops.grouped_wide_packed_codebook_linear(xx, codes, c, group_rows, b, relu=True),
                lambda xx, c, b: ops.grouped_codebook_linear(xx, codes.to_dense(), c, kdim, ncols, group_rows, b, relu=True, half_inputs=True)):
        leaves = [_cuda(x).to(tdt).requires_grad_(), _cuda(cen).requires_grad_(), _cuda(bias).requires_grad_()]
        y = run(*leaves)
        assert y.dtype == tdt and y.shape == (m, ncols)
        y.backward(_cuda(gy).to(tdt))
        grads.append([y.detach()] + [t.grad for t in leaves])
    (yw, dxw, dcw, dbw), (yb, dxb, dcb, dbb) = grads
    assert torch.equal(yw, yb) and (yw > 0).any() and (yw <= 0).any()
    assert dxw.dtype == tdt and dcw.dtype == dbw.dtype == torch.float32 and dcw.shape == cen.shape
    assert torch.equal(dcw, dcb) and torch.equal(dbw, dbb) and dcw.abs().sum() > 0
    g_eff = np.where(yw.double().cpu().numpy() > 0, gy.astype(np.float64), 0.0)
    c, c64 = _shape(m, kdim, ncols, k, group_rows), torch.from_numpy(cen).to(tdt).double().numpy()
    eps = {"f32": 0.0, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}[dtype]
    tol = 2.0 * ref.dx_bound(c, g_eff, lab, c64) + 2.0 * eps * np.abs(ref.dx64(c, g_eff, lab, c64))
    assert (np.abs(dxw.double().cpu().numpy() - dxb.double().cpu().numpy()) <= tol).all()
    with pytest.raises(TypeError):
        ops.grouped_wide_packed_codebook_linear(_cuda(x).to(torch.bfloat16), codes, _cuda(cen).to(torch.bfloat16), group_rows)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.grouped_wide_packed_codebook_matmul(_cuda(x), codes, _cuda(cen).requires_grad_(), group_rows)


class _Net(torch.nn.Module):
    """Dense 80 x 100 (groups of 32 rows: 32, 32, 16) -> Dense 100 x 10 (groups of 64), trainable group-wise byte layers of K = 17
    centres that are multiples of 1/2 up to 1, integer biases: on inputs of -1, 0, 1 every activation and gradient is exact in float32,
    whatever the order of the sums."""

    def __init__(self):
        super().__init__()
        rng = np.random.RandomState(5)
        lab = lambda n: _cuda(rng.randint(0, 17, size=n).astype(np.uint8))                       # noqa: E731
        cen, b = lambda g: _cuda((rng.randint(-2, 3, size=(g, 17)) / 2.0).astype(np.float32)), lambda n: _cuda(rng.randint(-2, 3, size=n).astype(np.float32))  # noqa: E731
        self.hidden = compressed.TrainableGroupedCompressedDense(80, 100, 32, lab(8000), cen(3), b(100), None, torch.relu)
        self.out = compressed.TrainableGroupedCompressedDense(100, 10, 64, lab(1000), cen(2), b(10), None, None)

    def get_config(self):
        return {"hidden": self.hidden, "out": self.out}

    def forward(self, x):
        return self.out(self.hidden(x))


def test_widened_trainable_layers_take_the_byte_layers_step():
    net = _Net().cuda()
    assert [type(l) for l in compressed.widen_grouped_layers(net).get_config().values()] == [compressed.TrainableGroupedCompressedDense] * 2
    wide = compressed.widen_grouped_layers(net, trainable=True)
    assert [type(l) for l in wide.get_config().values()] == [compressed.TrainableGroupedWidePackedCompressedDense] * 2
    assert type(compressed.widen_grouped_layers(net, "auto", trainable=True).out) is compressed.TrainableGroupedCompressedDense   # 10 columns: 32 bytes a row
    assert net.hidden.nbytes() - wide.hidden.nbytes() == 80 * (100 - 80)   # a row of 100 labels: 64 bytes of fields, 16 of plane
    packed = {n: l.packed.clone() for n, l in wide.get_config().items()}
    rng = np.random.RandomState(9)
    x, w = _cuda(rng.randint(-1, 2, size=(6, 80)).astype(np.float32)), _cuda(rng.choice([-1.0, 1.0], size=(6, 10)).astype(np.float32))
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
    h = net.hidden
    frozen = compressed.GroupedWidePackedCompressedDense.from_codes(h.kdim, h.ncols, h.group_rows, h.labels, h.centers.detach(), h.bias, h.activation)
    again = compressed.TrainableGroupedWidePackedCompressedDense.from_grouped_wide_packed(frozen)
    assert torch.equal(again.counts, h.counts) and torch.equal(again.packed, wide.hidden.packed)
    with pytest.raises(ValueError, match="17 <= K <= 64"):
        compressed.TrainableGroupedWidePackedCompressedDense.from_codes(80, 100, 32, h.labels, h.centers[:, :16])
