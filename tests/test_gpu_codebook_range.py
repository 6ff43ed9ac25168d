"""The codebook family across the float32 range (run with -m gpu): the centroid gradients (ops.codebook_centroid_grad,
ops.sparse_codebook_centroid_grad, ops.centroid_gradient), the forward passes and dx, at magnitudes from subnormal to the top of
the range, on every plan regime of the backward case lists.

Scaled exact data (tests/helpers/range_ref.py) must give the float64 formula bit for bit in float64 and float32(formula) in
float32, subnormal results, 0 and inf included; fitted layers scaled far from 1 stay within the bounds of DESIGN.md sections 12
and 13; a NaN or Inf gradient makes every centroid gradient NaN."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_compression_amd import synth  # noqa: E402
from tests.helpers import cbgrad_ref as dref  # noqa: E402
from tests.helpers import range_ref as rr  # noqa: E402
from tests.helpers import sparse_grad_ref as sref  # noqa: E402


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, ops

    _native.load()
    _, cus = ops.device_info()
    return ops, cus


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dense_labels(lab, lb, off=0):
    """The indices as uint8 / int16 starting ``off`` elements into a buffer with 16 spare bytes after them."""
    dt = torch.uint8 if lb == 1 else torch.int16
    host = lab.astype(np.uint8) if lb == 1 else lab.astype(np.uint16).view(np.int16)
    buf = torch.zeros(off + host.size + 16 // lb, dtype=dt, device="cuda")
    buf[off: off + host.size] = torch.from_numpy(np.ascontiguousarray(host).ravel()).cuda()
    return buf[off: off + host.size]


def _dense_case(case, seed):
    name, m, kdim, ncols, lb, k, off, _ = case
    x, g, c, lab = dref.case_data(case, seed)
    return x, g, c, lab, _dense_labels(lab, lb, off)


def _sparse_case(ops, case, seed):
    name, m, kdim, ncols, lb, k = case[:6]
    x, g, c, lab, z = sref.case_data(case, seed)
    codes = ops.pack_sparse_codes(_dense_labels(lab, lb), kdim, ncols, k, zero_symbol=z)
    return x, g, c, lab, codes


def _dc_both(ops, x, g, labels, k, kdim, ncols):
    xt, gt = _cuda(x), _cuda(g)
    return [ops.codebook_centroid_grad(xt, gt, labels, k, kdim, ncols, dtype=dt).cpu().numpy() for dt in (torch.float64, torch.float32)]


def _check_dc(ops, cus, m, kdim, ncols, lb, k, x, g, lab, got64, got32, label):
    """got64 / got32 against the exact float64 formula (all NaN on the NaN side of the shift rule, all 0 for a zero maximum)."""
    t = ops.cbmm_dc_plan(m, kdim, ncols, lb, k, cus)["terms_log2"]
    _, flag = ops.cbgrad_shift(m, float(np.abs(x).max()), float(np.abs(g).max()), t)
    if flag == ops.CBGRAD_NONFINITE:
        assert np.isnan(got64).all() and np.isnan(got32).all(), label
        return flag
    want = dref.dc64(x, g, lab, k)
    if flag == ops.CBGRAD_ZERO:
        assert not want.any()
    assert np.array_equal(got64, want), (label, np.flatnonzero(got64 != want)[:5])
    assert np.array_equal(got32, rr.f32_of(want)), label
    return flag


# ------------------------------------------------------------------ dc: scaled exact data
@pytest.mark.parametrize("ab", rr.DC_EXPONENTS, ids=[e[0] for e in rr.DC_EXPONENTS])
@pytest.mark.parametrize("case", rr.DENSE_CASES, ids=[c[0] for c in rr.DENSE_CASES])
def test_dense_dc_is_the_float64_formula_at_every_scale(env, case, ab):
    ops, cus = env
    name, m, kdim, ncols, lb, k = case[:6]
    _, a, b = ab
    xi, gi, _, lab, labels = _dense_case(case, seed=len(name) * 7 + m)
    x, g = rr.scale(xi, a), rr.scale(gi, b)
    got64, got32 = _dc_both(ops, x, g, labels, k, kdim, ncols)
    flag = _check_dc(ops, cus, m, kdim, ncols, lb, k, x, g, lab, got64, got32, (name, a, b))
    assert flag == (ops.CBGRAD_OK if xi.any() and gi.any() else ops.CBGRAD_ZERO)


@pytest.mark.parametrize("case", rr.DENSE_CASES, ids=[c[0] for c in rr.DENSE_CASES])
def test_dense_dc_at_the_top_of_the_range(env, case):
    ops, cus = env
    name, m, kdim, ncols, lb, k = case[:6]
    xi, gi, _, lab, labels = _dense_case(case, seed=len(name) * 7 + m)
    for below, want_flag in ((True, ops.CBGRAD_OK), (False, ops.CBGRAD_NONFINITE)):
        want_flag = want_flag if xi.any() and gi.any() else ops.CBGRAD_ZERO
        e = rr.top_exponent(m, xi, gi, below)
        x, g = rr.scale(xi, e // 2), rr.scale(gi, e - e // 2)
        got64, got32 = _dc_both(ops, x, g, labels, k, kdim, ncols)
        assert _check_dc(ops, cus, m, kdim, ncols, lb, k, x, g, lab, got64, got32, (name, e)) == want_flag, (name, e)


@pytest.mark.parametrize("case", rr.DENSE_CASES[:3] + rr.DENSE_CASES[-3:], ids=[c[0] for c in rr.DENSE_CASES[:3] + rr.DENSE_CASES[-3:]])
def test_dense_dc_of_a_zero_operand_is_zero_at_every_scale(env, case):
    ops, _ = env
    name, m, kdim, ncols, lb, k = case[:6]
    xi, gi, _, lab, labels = _dense_case(case, seed=len(name) * 7 + m)
    for _, a, b in rr.DC_EXPONENTS:
        for x, g in ((np.zeros_like(xi), rr.scale(gi, b)), (rr.scale(xi, a), np.zeros_like(gi))):
            for got in _dc_both(ops, x, g, labels, k, kdim, ncols):
                assert (got == 0).all() and not np.signbit(got).any(), (name, a, b)


@pytest.mark.parametrize("ab", rr.DC_EXPONENTS, ids=[e[0] for e in rr.DC_EXPONENTS])
@pytest.mark.parametrize("case", rr.SPARSE_CASES, ids=[c[0] for c in rr.SPARSE_CASES])
def test_sparse_dc_is_the_formula_and_the_dense_dc_at_every_scale(env, case, ab):
    ops, cus = env
    name, m, kdim, ncols, lb, k = case[:6]
    _, a, b = ab
    xi, gi, _, lab, codes = _sparse_case(ops, case, seed=len(name) * 7 + m)
    x, g = rr.scale(xi, a), rr.scale(gi, b)
    xt, gt = _cuda(x), _cuda(g)
    got = [ops.sparse_codebook_centroid_grad(xt, gt, codes, dtype=dt) for dt in (torch.float64, torch.float32)]
    dense = codes.to_dense()
    for dt, v in zip((torch.float64, torch.float32), got):
        assert torch.equal(v, ops.codebook_centroid_grad(xt, gt, dense, k, kdim, ncols, dtype=dt)), (name, a, b)
    flag = _check_dc(ops, cus, m, kdim, ncols, lb, k, x, g, lab, got[0].cpu().numpy(), got[1].cpu().numpy(), (name, a, b))
    assert flag == (ops.CBGRAD_ZERO if not gi.any() or not xi.any() else ops.CBGRAD_OK)


@pytest.mark.parametrize("case", rr.SPARSE_CASES, ids=[c[0] for c in rr.SPARSE_CASES])
def test_sparse_dc_at_the_top_of_the_range(env, case):
    ops, cus = env
    name, m, kdim, ncols, lb, k = case[:6]
    xi, gi, _, lab, codes = _sparse_case(ops, case, seed=len(name) * 7 + m)
    dense = codes.to_dense()
    for below, want_flag in ((True, ops.CBGRAD_OK), (False, ops.CBGRAD_NONFINITE)):
        want_flag = want_flag if xi.any() and gi.any() else ops.CBGRAD_ZERO
        e = rr.top_exponent(m, xi, gi, below)
        x, g = rr.scale(xi, e // 2), rr.scale(gi, e - e // 2)
        xt, gt = _cuda(x), _cuda(g)
        got = [ops.sparse_codebook_centroid_grad(xt, gt, codes, dtype=dt) for dt in (torch.float64, torch.float32)]
        for dt, v in zip((torch.float64, torch.float32), got):
            want = ops.codebook_centroid_grad(xt, gt, dense, k, kdim, ncols, dtype=dt)
            assert torch.equal(torch.nan_to_num(v, nan=7.0), torch.nan_to_num(want, nan=7.0)), (name, e)
        flag = _check_dc(ops, cus, m, kdim, ncols, lb, k, x, g, lab, got[0].cpu().numpy(), got[1].cpu().numpy(), (name, e))
        assert flag == want_flag, (name, e)


# ------------------------------------------------------------------ dc and dx: fitted layers far from 1
@functools.lru_cache(maxsize=None)
def _fit(shape, seed, bits, mode):
    from neural_network_compression_amd import pipeline

    w = synth.weights(shape, seed)
    res = pipeline.compress_layer(torch.from_numpy(w.copy()).cuda(), q=1, bits=bits, mode=mode)
    return res.model.cluster_centers_.ravel().astype(np.float32), res.model.labels_.reshape(shape).astype(np.int64)


@pytest.mark.parametrize("e", [-70, 50])
@pytest.mark.parametrize("m", [1, 16, 300])
@pytest.mark.parametrize("shape,bits,mode,lb", [((784, 300), 5, "linear", 1), ((300, 100), 9, "density", 2)])
def test_fitted_data_scaled_far_from_one_is_within_the_bounds(env, e, m, shape, bits, mode, lb):
    ops, cus = env
    c, lab = _fit(shape, 4000, bits, mode)
    k = c.size
    kdim, ncols = shape
    labels = _dense_labels(lab, lb)
    rng = np.random.RandomState(m)
    x = rr.scale((rng.randn(m, kdim) * 0.7).astype(np.float32), e)
    g = rr.scale((rng.randn(m, ncols) * 1e-2).astype(np.float32), e)
    dx = ops.codebook_matmul_dx(_cuda(g), labels, _cuda(c), kdim, ncols).cpu().numpy()
    assert np.all(np.abs(dx - dref.dx64(g, lab, c)) <= dref.dx_bound(g, lab, c))
    t = ops.cbmm_dc_plan(m, kdim, ncols, lb, k, cus)["terms_log2"]
    S, flag = ops.cbgrad_shift(m, np.abs(x).max(), np.abs(g).max(), t)
    assert flag == ops.CBGRAD_OK
    want = dref.dc64(x, g, lab, k)
    codes = ops.pack_sparse_codes(labels, kdim, ncols, k)
    for dt, f32 in ((torch.float64, False), (torch.float32, True)):
        dc = ops.codebook_centroid_grad(_cuda(x), _cuda(g), labels, k, kdim, ncols, dtype=dt)
        # (a float32 result also rounds in float32's subnormal range: half its step, 2^-150)
        bound = dref.dc_bound(x, g, lab, k, S, f32_out=f32) + (2.0 ** -150 if f32 else 0.0)
        assert np.all(np.abs(dc.cpu().numpy().astype(np.float64) - want) <= bound), (dt, e)
        assert torch.equal(ops.sparse_codebook_centroid_grad(_cuda(x), _cuda(g), codes, dtype=dt), dc)


# ------------------------------------------------------------------ forward and dx: subnormal products, overflow, just below it
def _scaled_operands(xi, ci, ex, ec):
    """x_int * 2^ex and centres (ci in quarters) * 2^ec: every product is an integer times 2^(ex + ec - 2)."""
    return rr.scale(xi, ex), rr.scale(ci, ec)


def _positive(rng, shape, top=3):
    return rng.randint(1, top + 1, size=shape).astype(np.float32)


def _dense_fwd_dx(ops, x, g, c, labels, kdim, ncols):
    y = ops.codebook_matmul(_cuda(x), labels, _cuda(c), kdim, ncols).cpu().numpy()
    dx = ops.codebook_matmul_dx(_cuda(g), labels, _cuda(c), kdim, ncols).cpu().numpy()
    return y, dx


@pytest.mark.parametrize("case", rr.DENSE_CASES, ids=[c[0] for c in rr.DENSE_CASES])
def test_dense_forward_and_dx_subnormal_products_and_overflow(env, case):
    ops, _ = env
    name, m, kdim, ncols, lb, k = case[:6]
    xi, gi, ci, lab, labels = _dense_case(case, seed=len(name) * 7 + m)
    W = dref.decoded(lab, ci)
    # products that are representable subnormals: the exact value, whatever the path
    for ex, ec in ((-70, -68), (-75, -71)):
        x, c = _scaled_operands(xi, ci, ex, ec)
        g = rr.scale(gi, ex)
        y, dx = _dense_fwd_dx(ops, x, g, c, labels, kdim, ncols)
        assert np.array_equal(y, rr.f32_of(x.astype(np.float64) @ dref.decoded(lab, c))), (name, ex, ec)
        assert np.array_equal(dx, rr.f32_of(dref.dx64(g, lab, c))), (name, ex, ec)
        assert np.abs(y[y != 0]).min(initial=1.0) < rr.FLT_MIN or not y.any()
    # just below overflow: every partial sum stays below FLT_MAX, the result is exact
    ey = rr.grid_exponent(np.abs(xi) @ np.abs(W) * 4)
    edx = rr.grid_exponent(np.abs(gi) @ np.abs(W).T * 4)
    x, c = _scaled_operands(xi, ci, ey // 2, ey - ey // 2 + 2)
    y = ops.codebook_matmul(_cuda(x), labels, _cuda(c), kdim, ncols).cpu().numpy()
    want = x.astype(np.float64) @ dref.decoded(lab, c)
    assert np.isfinite(y).all() and np.array_equal(y, rr.f32_of(want)), name
    g, c = _scaled_operands(gi, ci, edx // 2, edx - edx // 2 + 2)
    dx = ops.codebook_matmul_dx(_cuda(g), labels, _cuda(c), kdim, ncols).cpu().numpy()
    assert np.isfinite(dx).all() and np.array_equal(dx, rr.f32_of(dref.dx64(g, lab, c))), name
    # every term of one sign, the exact result 0 or at least 2^129 >= 2 FLT_MAX: inf, whatever the order
    rng = np.random.RandomState(m + kdim)
    xp, gp, cp = _positive(rng, xi.shape), _positive(rng, gi.shape), _positive(rng, ci.shape, 8)
    x, c = _scaled_operands(xp, cp, 66, 65)
    g = rr.scale(gp, 66)
    y, dx = _dense_fwd_dx(ops, x, g, c, labels, kdim, ncols)
    wy, wdx = x.astype(np.float64) @ dref.decoded(lab, c), dref.dx64(g, lab, c)
    assert (np.isinf(wy) | (wy == 0) | (wy >= 2 * rr.FLT_MAX)).all()
    assert np.array_equal(y, rr.f32_of(wy)) and np.array_equal(dx, rr.f32_of(wdx)), name
    assert np.isposinf(y).any() and np.isposinf(dx).any()


@pytest.mark.parametrize("case", rr.SPARSE_CASES, ids=[c[0] for c in rr.SPARSE_CASES])
def test_sparse_forward_and_dx_subnormal_products_and_overflow(env, case):
    ops, _ = env
    name, m, kdim, ncols, lb, k = case[:6]
    xi, gi, ci, lab, codes = _sparse_case(ops, case, seed=len(name) * 7 + m)
    z = codes.zero_symbol

    def run(x, g, c):
        y = ops.sparse_codebook_matmul(_cuda(x), codes, _cuda(c)).cpu().numpy()
        dx = ops.sparse_codebook_matmul_dx(_cuda(g), codes, _cuda(c)).cpu().numpy()
        return y, dx

    def mags(v, transpose):
        """Bounds of every partial sum of the sparse formula (forward: v = x; dx: v = g), in steps of the integer grid."""
        D, cz = sref.stored_d(lab, ci * 4, z)
        return np.abs(v) @ np.abs(D.T if transpose else D) + abs(cz) * np.abs(v).sum(axis=1, keepdims=True)

    for ex, ec in ((-70, -68), (-75, -71)):
        x, c = _scaled_operands(xi, ci, ex, ec)
        g = rr.scale(gi, ex)
        y, dx = run(x, g, c)
        assert np.array_equal(y, rr.f32_of(x.astype(np.float64) @ sref.decoded(lab, c))), (name, ex, ec)
        assert np.array_equal(dx, rr.f32_of(sref.dx64(g, lab, c, z))), (name, ex, ec)
    ey, edx = rr.grid_exponent(mags(xi, False)), rr.grid_exponent(mags(gi, True))
    x, c = _scaled_operands(xi, ci, ey // 2, ey - ey // 2 + 2)
    y = ops.sparse_codebook_matmul(_cuda(x), codes, _cuda(c)).cpu().numpy()
    assert np.isfinite(y).all() and np.array_equal(y, rr.f32_of(x.astype(np.float64) @ sref.decoded(lab, c))), name
    g, c = _scaled_operands(gi, ci, edx // 2, edx - edx // 2 + 2)
    dx = ops.sparse_codebook_matmul_dx(_cuda(g), codes, _cuda(c)).cpu().numpy()
    assert np.isfinite(dx).all() and np.array_equal(dx, rr.f32_of(sref.dx64(g, lab, c, z))), name
    # one sign: positive operands and c_z = 0, so every term of the sparse formula is >= 0
    rng = np.random.RandomState(m + kdim)
    xp, gp, cp = _positive(rng, xi.shape), _positive(rng, gi.shape), _positive(rng, ci.shape, 8)
    if z < k:
        cp[z] = 0.0
    x, c = _scaled_operands(xp, cp, 66, 65)
    g = rr.scale(gp, 66)
    y, dx = run(x, g, c)
    wy, wdx = x.astype(np.float64) @ sref.decoded(lab, c), sref.dx64(g, lab, c, z)
    assert np.array_equal(y, rr.f32_of(wy)) and np.array_equal(dx, rr.f32_of(wdx)), name


# ------------------------------------------------------------------ ops.centroid_gradient
def _cg_data(n, k, lb, seed, oob=False):
    rng = np.random.RandomState(seed)
    g = (rng.randn(n) * 1e-3).astype(np.float32)
    g[::7] = 0
    top = (256 if lb == 1 else k + 40) if oob else k
    labels = rng.randint(0, top, size=n)
    lab_t = _cuda(labels.astype(np.uint8) if lb == 1 else labels.astype(np.uint16).view(np.int16))
    return g, labels, lab_t


def _cg_want(ops, g, labels, k):
    S = ops.fix_shift(float(np.abs(g).max()), g.size)
    ok = labels < k
    q = np.rint(np.ldexp(g[ok].astype(np.float64), S)).astype(np.int64)
    want = np.zeros(k, dtype=np.int64)
    np.add.at(want, labels[ok], q)
    return np.ldexp(want.astype(np.float64), -S)


@pytest.mark.parametrize("n,k,lb", [(1000, 4, 1), (30_000, 256, 1), (50_000, 1025, 2)])
@pytest.mark.parametrize("bad", ["nan", "+inf", "-inf", "+inf_-inf"])
def test_centroid_gradient_of_a_non_finite_gradient_is_all_nan(env, n, k, lb, bad):
    ops, _ = env
    g, labels, lab_t = _cg_data(n, k, lb, n + k)
    i, j = 5, int(np.flatnonzero(labels != labels[5])[0])        # two members of different clusters
    if bad == "nan":
        g[i] = np.nan
    elif bad == "+inf":
        g[i] = np.inf
    elif bad == "-inf":
        g[i] = -np.inf
    else:
        g[i], g[j] = np.inf, -np.inf
    out = ops.centroid_gradient(_cuda(g), lab_t, k)
    assert out.dtype == torch.float64 and out.shape == (k,)
    assert torch.isnan(out).all(), bad


@pytest.mark.parametrize("e", [100, -120, -135])
@pytest.mark.parametrize("n,k,lb", [(1000, 4, 1), (235_200, 33, 1), (50_000, 1025, 2)])
def test_centroid_gradient_is_the_exact_fixed_point_sum_far_from_one(env, n, k, lb, e):
    ops, _ = env
    g, labels, lab_t = _cg_data(n, k, lb, n + k + e)
    g = np.ldexp(g.astype(np.float64), e).astype(np.float32)   # (below 2^-126 the values round to float32's subnormal grid)
    if e < 0:
        assert 0 < np.abs(g).max() < rr.FLT_MIN                 # max |grad| subnormal
    out = ops.centroid_gradient(_cuda(g), lab_t, k).cpu().numpy()
    assert np.array_equal(out, _cg_want(ops, g, labels, k)), e


@pytest.mark.parametrize("k,lb", [(16, 1), (300, 2)])
def test_centroid_gradient_ignores_indices_at_or_above_k(env, k, lb):
    ops, _ = env
    g, labels, lab_t = _cg_data(20_000, k, lb, k, oob=True)
    assert (labels >= k).any()
    out = ops.centroid_gradient(_cuda(g), lab_t, k).cpu().numpy()
    assert np.array_equal(out, _cg_want(ops, g, labels, k))


# ------------------------------------------------------------------ trainable layers with a quantized bias
def _model(c, labels):
    from types import SimpleNamespace

    return SimpleNamespace(cluster_centers_=np.asarray(c, dtype=np.float32).reshape(-1, 1), labels_compact_=labels)


@pytest.mark.parametrize("sparse", [False, True])
def test_a_nan_loss_gives_nan_kernel_and_bias_centre_gradients(env, sparse):
    from neural_network_compression_amd import compressed
    from neural_network_compression_amd.neural_networks.layers import Dense

    torch.manual_seed(5)
    dense = Dense(120, 40).cuda()
    rng = np.random.RandomState(6)
    lab = sref.labels_for(rng, 120, 40, 16, 1, 0.3, 0)
    c = (rng.randn(16) * 0.1).astype(np.float32)
    c[0] = 0.0
    blab = rng.randint(0, 4, size=40)
    bc = (rng.randn(4) * 0.1).astype(np.float32)
    wm, bm = _model(c, _cuda(lab.ravel().astype(np.uint8))), _model(bc, _cuda(blab.astype(np.uint8)))
    layer = compressed.TrainableSparseCompressedDense.from_dense(dense, wm, bm) if sparse else compressed._trainable(dense, wm, bm)
    assert isinstance(layer, compressed.TrainableSparseCompressedDense if sparse else compressed.TrainableCompressedDense)
    assert layer.bias_centers is not None
    x = torch.randn(8, 120, device="cuda")
    loss = layer(x).sum() * float("nan")
    loss.backward()
    assert torch.isnan(layer.centers.grad).all()
    assert torch.isnan(layer.bias_centers.grad).all()
