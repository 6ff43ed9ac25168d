"""The backward pass of the group-wise codebook layer from the bitmap-sparse form of its indices (nnc_cbsp_grouped_dx_f32 /
nnc_cbsp_grouped_dc_f32, csrc/nnc_cbspgrad_grouped.hip) through ops.grouped_sparse_codebook_matmul_dx /
grouped_sparse_codebook_centroid_grad / grouped_sparse_codebook_linear, TrainableGroupedSparseCompressedDense,
compress_network_trainable_grouped(sparse=) and Trainer.fine_tune_grouped(sparse=) (run with -m gpu).

Every case of tests/helpers/grouped_sparse_grad_ref.py, bit for bit unless stated: dc against ops.grouped_codebook_centroid_grad on the
unpacked labels (float64 and float32; all NaN on an Inf in x, 0 on g = 0); dx group by group against ops.sparse_codebook_matmul_dx on
the same buffer read with the group's z and table; one group against the ungrouped sparse ops; exact data against the float64 formula
and the byte grouped dx; float data within the derived bound of section 13 taken per group; an Inf in g at a skipped column; sentinel
frames around dx, dc and a workspace of exactly the queried size; autograd against the byte grouped layer; the peak allocation of a
backward; the layer, the network function and one epoch of fine_tune_grouped(sparse=True) on a pruned LeNet-300-100.
(The file name sorts behind every earlier GPU test file, so the suite's order up to here is what it was.)"""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_compression_amd import synth  # noqa: E402
from tests.helpers import cbgrad_ref, grouped_grad_ref, sparse_ref  # noqa: E402
from tests.helpers import grouped_sparse_grad_ref as ref  # noqa: E402
from tests.helpers.grouped_sparse_grad_ref import CASES, IDS  # noqa: E402

fwd = ref.fwd
PAD, WS_PAD = 37, 64          # sentinel elements on each side of an output (odd: it is only element-aligned) and bytes around a workspace
SENT32, SENT64, WS_BYTE = 0x7FA5A5A5, 0x7FF8A5A5A5A5A5A5, 0xA5   # NaN patterns no result takes, and the workspace's fill


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, ops

    _, cus = ops.device_info()
    assert cus >= 1
    return types.SimpleNamespace(ops=ops, cus=cus, lib=_native.load(), nat=_native)


def _dev(host):
    return torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).cuda()


def _dev_labels(lab, off=0):
    """The indices as uint8 starting ``off`` bytes into a larger buffer."""
    host = np.ascontiguousarray(np.asarray(lab).ravel().astype(np.uint8))
    buf = torch.zeros(off + host.size + 16, dtype=torch.uint8, device="cuda")
    buf[off: off + host.size] = torch.from_numpy(host).cuda()
    return buf[off: off + host.size]


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.fixture(scope="module")
def case_data(env):
    """Per case, made once and left unchanged: exact and float data on the host, the packed form and the unpacked labels on the device."""
    out = []
    for ci, c in enumerate(CASES):
        lab, zs, x, g, cen = ref.exact_data(c, 300 + ci, ci)
        xf, gf, cf = ref.float_data(c, zs, 300 + ci)
        lab_t = _dev_labels(lab, c["off"])
        assert lab_t.storage_offset() == c["off"]
        zs_t = torch.from_numpy(zs).cuda()
        codes = env.ops.pack_grouped_sparse_codes(lab_t, c["kdim"], c["ncols"], c["k"], c["group_rows"], zero_symbols=zs_t)
        assert codes.nnz == int(fwd.keep_mask(lab, zs, c["group_rows"]).sum()) and (codes.nnz == 0) == c["pruned"]
        unpacked = codes.to_dense()
        assert np.array_equal(unpacked.cpu().numpy().reshape(lab.shape), lab.astype(np.uint8))
        out.append(dict(lab=lab, zs=zs, x=x, g=g, cen=cen, xf=xf, gf=gf, cf=cf, codes=codes, unpacked=unpacked))
    return out


def _plans(env, c):
    a = (c["m"], c["kdim"], c["ncols"], c["k"], c["group_rows"], env.cus)
    return env.ops.cbsp_grouped_dx_plan(*a), env.ops.cbsp_grouped_dc_plan(*a)


def test_the_case_list_hits_every_regime_and_group_walk_at_this_device(env):
    seen, feats = set(), set()
    for c in CASES:
        dx, dc = _plans(env, c)
        seen |= ref.regimes_of(dx, dc)
        feats |= ref.features_of(c, "dx", dx) | ref.features_of(c, "dc", dc)
    for m, kdim, ncols in ref.EMPTY:
        seen |= ref.regimes_of(env.ops.cbsp_grouped_dx_plan(m, kdim, ncols, 16, 32, env.cus), env.ops.cbsp_grouped_dc_plan(m, kdim, ncols, 16, 32, env.cus))
    assert ref.required_regimes() <= seen, ref.required_regimes() - seen
    assert ref.required_features() <= feats, ref.required_features() - feats


# ------------------------------------------------------------------ check 1: dc is the byte grouped dc on the unpacked labels
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_dc_is_the_byte_grouped_dc_on_the_unpacked_labels(env, case_data, ci):
    c, d = CASES[ci], case_data[ci]
    ops = env.ops
    a = (c["k"], c["kdim"], c["ncols"], c["group_rows"])
    for x, g in ((d["xf"], d["gf"]), (d["x"], d["g"])):
        x_t, g_t = _dev(x), _dev(g)
        for dt in (torch.float64, torch.float32):
            got = ops.grouped_sparse_codebook_centroid_grad(x_t, g_t, d["codes"], dtype=dt)
            want = ops.grouped_codebook_centroid_grad(x_t, g_t, d["unpacked"], *a, dtype=dt)
            assert got.shape == (fwd.groups_of(c), c["k"]) and got.dtype == dt
            assert torch.equal(_bits(got), _bits(want)), dt
            assert torch.equal(_bits(got), _bits(ops.grouped_sparse_codebook_centroid_grad(x_t, g_t, d["codes"], dtype=dt)))   # the same call, the same bits
    # the all-NaN rule (an Inf in x) and dc = 0 on a zero maximum (g = 0)
    x_t, g_t = _dev(d["xf"]), _dev(d["gf"])
    xi = x_t.clone()
    xi[c["m"] - 1, c["kdim"] // 2] = float("inf")
    for dt in (torch.float64, torch.float32):
        nan = ops.grouped_sparse_codebook_centroid_grad(xi, g_t, d["codes"], dtype=dt)
        assert bool(torch.isnan(nan).all())
        assert torch.equal(_bits(nan), _bits(ops.grouped_codebook_centroid_grad(xi, g_t, d["unpacked"], *a, dtype=dt)))
        zero = ops.grouped_sparse_codebook_centroid_grad(x_t, torch.zeros_like(g_t), d["codes"], dtype=dt)
        assert not bool(zero.any())
        assert torch.equal(_bits(zero), _bits(ops.grouped_codebook_centroid_grad(x_t, torch.zeros_like(g_t), d["unpacked"], *a, dtype=dt)))


# ------------------------------------------------------------------ check 2: dx, group by group, is the ungrouped sparse dx
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_dx_group_by_group_is_the_ungrouped_sparse_dx_on_the_same_buffer(env, case_data, ci):
    c, d = CASES[ci], case_data[ci]
    ops, rows = env.ops, c["group_rows"]
    codes = d["codes"]
    g_t, cen_t = _dev(d["gf"]), _dev(d["cf"])
    dx = ops.grouped_sparse_codebook_matmul_dx(g_t, codes, cen_t)
    assert dx.shape == (c["m"], c["kdim"]) and dx.dtype == torch.float32
    for q, z in enumerate(d["zs"]):
        one = ops.SparseCodes(codes.buf, c["kdim"], c["ncols"], c["k"], int(z), 1, codes.nnz)
        want = ops.sparse_codebook_matmul_dx(g_t, one, cen_t[q].contiguous())
        lo, hi = q * rows, min(c["kdim"], (q + 1) * rows)
        assert torch.equal(_bits(dx[:, lo:hi]), _bits(want[:, lo:hi])), q   # (the other columns of `want` mean nothing)
    assert torch.equal(_bits(dx), _bits(ops.grouped_sparse_codebook_matmul_dx(g_t, codes, cen_t)))


# ------------------------------------------------------------------ check 3: one group is the ungrouped sparse backward
ONE_GROUP = [(1, 112, 70, 16), (2, 200, 1, 3), (4, 130, 600, 256), (8, 63, 260, 16), (16, 112, 130, 16),   # stream, one and several blocks
             (17, 112, 130, 16), (17, 300, 260, 256), (260, 100, 65, 3)]                                   # tiled: direct, dx split, dc split


@pytest.mark.parametrize("m,kdim,ncols,k", ONE_GROUP, ids=[f"m{a}-kd{b}-n{c}-k{d}" for a, b, c, d in ONE_GROUP])
def test_one_group_is_the_ungrouped_sparse_backward(env, m, kdim, ncols, k):
    ops = env.ops
    rng = np.random.RandomState(m * 1000 + kdim)
    z = 3 % k
    lab_t = _dev_labels(sparse_ref.labels_at_density(rng, kdim, ncols, k, 0.15, z), 1)
    rows = -(-kdim // 32) * 32 + 32 * (m % 2)                      # group_rows >= kdim: kdim rounded up, and beyond
    gcodes = ops.pack_grouped_sparse_codes(lab_t, kdim, ncols, k, rows, zero_symbols=torch.tensor([z], dtype=torch.uint8, device="cuda"))
    scodes = ops.pack_sparse_codes(lab_t, kdim, ncols, k, zero_symbol=z)
    x_t, g_t = _dev(rng.standard_normal((m, kdim))), _dev(rng.standard_normal((m, ncols)))
    cen = rng.standard_normal(k).astype(np.float32)
    for cz_zero in (True, False):
        cc = cen.copy()
        if cz_zero:
            cc[z] = 0.0
        cen_t = _dev(cc)
        assert torch.equal(_bits(ops.grouped_sparse_codebook_matmul_dx(g_t, gcodes, cen_t.view(1, k))), _bits(ops.sparse_codebook_matmul_dx(g_t, scodes, cen_t)))
    for dt in (torch.float64, torch.float32):
        got = ops.grouped_sparse_codebook_centroid_grad(x_t, g_t, gcodes, dtype=dt)
        assert torch.equal(_bits(got.view(-1)), _bits(ops.sparse_codebook_centroid_grad(x_t, g_t, scodes, dtype=dt)))


# ------------------------------------------------------------------ check 4: exact data
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_exact_data_is_the_float64_formula_and_the_byte_grouped_dx(env, case_data, ci):
    c, d = CASES[ci], case_data[ci]
    ops = env.ops
    want = ref.dx64(d["g"], d["lab"], d["cen"], d["zs"], c["group_rows"])
    g_t, cen_t = _dev(d["g"]), _dev(d["cen"])
    dx = ops.grouped_sparse_codebook_matmul_dx(g_t, d["codes"], cen_t)
    got = dx.cpu().numpy()
    assert np.array_equal(got.astype(np.float64), want), float(np.abs(got - want).max())
    assert torch.equal(dx, ops.grouped_codebook_matmul_dx(g_t, d["unpacked"], cen_t, c["kdim"], c["ncols"], c["group_rows"]))


# ------------------------------------------------------------------ check 5: float data within the derived bound
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_float_data_dx_is_within_the_derived_bound(env, case_data, ci):
    c, d = CASES[ci], case_data[ci]
    want, bound = ref.dx_bound(d["gf"], d["lab"], d["cf"], d["zs"], c["group_rows"])
    dx = env.ops.grouped_sparse_codebook_matmul_dx(_dev(d["gf"]), d["codes"], _dev(d["cf"]))
    err = np.abs(dx.cpu().numpy().astype(np.float64) - want)
    print(f"{ref.case_id(c)}: largest err / bound = {float((err / bound).max()):.4f}")
    assert np.all(err <= bound)


# ------------------------------------------------------------------ check 6: an Inf in g at a skipped column
@pytest.mark.parametrize("m", [1, 17])
def test_inf_in_g_at_a_skipped_column(env, m):
    ops = env.ops
    rng = np.random.RandomState(5 + m)
    kdim, ncols, k, rows = 96, 70, 16, 32
    zs = np.array([3, 5, 7], dtype=np.uint8)
    lab = np.concatenate([sparse_ref.labels_at_density(rng, rows, ncols, k, 0.3, int(z)) for z in zs], axis=0)
    cols = (11, 40)
    for col in cols:
        lab[0:32, col], lab[32:64, col], lab[64:96, col] = 3, 5, 7     # these columns are skipped in every row
    cen = (rng.standard_normal((3, k)) + 2.0).astype(np.float32)
    cen[1, 5] = 0.0                                                # c_{z_1} == 0 exactly; groups 0 and 2 keep their rank-1 terms
    codes = ops.pack_grouped_sparse_codes(_dev_labels(lab), kdim, ncols, k, rows, zero_symbols=torch.from_numpy(zs).cuda())
    cen_t = _dev(cen)
    base = rng.standard_normal((m, ncols)).astype(np.float32)
    gz = base.copy()
    gz[m - 1, list(cols)] = 0.0
    r64, bound = ref.dx_bound(gz, lab, cen, zs, rows)
    for infs in ((np.inf,), (np.inf, -np.inf)):                    # one Inf: the row sum of g is Inf; two of opposite sign: it is NaN
        g = base.copy()
        g[m - 1, list(cols[: len(infs)])] = infs
        g_t = _dev(g)
        dx = ops.grouped_sparse_codebook_matmul_dx(g_t, codes, cen_t).cpu().numpy()
        byte = ops.grouped_codebook_matmul_dx(g_t, _dev_labels(lab), cen_t, kdim, ncols, rows).cpu().numpy()
        assert np.isfinite(dx[:, 32:64]).all()                     # c_z == 0: the skipped weights are absent, Inf meets no 0
        assert np.isnan(byte[m - 1, 32:64]).all()                  # the byte form multiplies Inf by the 0 centre
        rest = np.concatenate([dx[m - 1, :32], dx[m - 1, 64:]])    # c_z != 0: c_z * the row sum
        assert np.isinf(rest).all() if len(infs) == 1 else np.isnan(rest).all()
        want = ref.dx64(g, lab, cen, zs, rows)
        assert np.array_equal(np.isnan(dx), np.isnan(want)) and np.array_equal(np.isinf(dx), np.isinf(want))
        assert np.isfinite(dx[: m - 1]).all()
        assert np.all(np.abs(dx[:, 32:64].astype(np.float64) - r64[:, 32:64]) <= bound[:, 32:64])
    # a NaN centre as c_z propagates: c != 0 holds for a NaN
    cen[1, 5] = np.nan
    gf = _dev(gz)
    dxn = ops.grouped_sparse_codebook_matmul_dx(gf, codes, _dev(cen)).cpu().numpy()
    assert np.isnan(dxn[:, 32:64]).all() and np.isfinite(dxn[:, :32]).all() and np.isfinite(dxn[:, 64:]).all()


# ------------------------------------------------------------------ check 7: sentinel frames, the same bits twice, m = 16 against m = 17
def _framed(units, tdtype, sent):
    buf = torch.full((units + 2 * PAD,), sent, dtype=tdtype, device="cuda")
    return buf, buf[PAD: PAD + units]


def _frame_intact(buf, units, sent, pad=PAD):
    return bool((buf[:pad] == sent).all()) and bool((buf[pad + units:] == sent).all())


def _workspace(nbytes):
    buf = torch.full((nbytes + 2 * WS_PAD,), WS_BYTE, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    return buf, buf.data_ptr() + WS_PAD


def _raw_dx(env, c, codes, g_t, cen_t):
    L, m, kdim, ncols = env.lib, c["m"], c["kdim"], c["ncols"]
    need = int(L.nnc_cbsp_grouped_dx_workspace_bytes(m, kdim, ncols))
    assert need == _plans(env, c)[0]["workspace"]
    obuf, out = _framed(m * kdim, torch.int32, SENT32)
    wbuf, ws = _workspace(need)
    env.nat.check(L.nnc_cbsp_grouped_dx_f32(g_t.data_ptr(), m, kdim, codes.buf.data_ptr(), codes.buf.numel(), ncols, codes.zero_symbols.data_ptr(), codes.nnz,
                                            cen_t.data_ptr(), c["k"], c["group_rows"], out.data_ptr(), ws, need, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert _frame_intact(obuf, m * kdim, SENT32), "a store outside dx"
    assert _frame_intact(wbuf, need, WS_BYTE, WS_PAD), "a store outside the dx workspace"
    assert not bool((out == SENT32).any()), "a dx element left unwritten"
    return out.clone()


def _raw_dc(env, c, codes, x_t, g_t, f64):
    L, m, kdim, ncols, k = env.lib, c["m"], c["kdim"], c["ncols"], c["k"]
    need = int(L.nnc_cbsp_grouped_dc_workspace_bytes(m, kdim, ncols, k, c["group_rows"]))
    n = fwd.groups_of(c) * k
    assert need == 64 + 8 * n == _plans(env, c)[1]["workspace"]
    obuf, out = _framed(n, torch.int64, SENT64) if f64 else _framed(n, torch.int32, SENT32)
    wbuf, ws = _workspace(need)
    env.nat.check(L.nnc_cbsp_grouped_dc_f32(x_t.data_ptr(), g_t.data_ptr(), m, kdim, codes.buf.data_ptr(), codes.buf.numel(), ncols,
                                            codes.zero_symbols.data_ptr(), codes.nnz, k, c["group_rows"], out.data_ptr(), f64, ws, need,
                                            torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    sent = SENT64 if f64 else SENT32
    assert _frame_intact(obuf, n, sent), "a store outside dc"
    assert _frame_intact(wbuf, need, WS_BYTE, WS_PAD), "a store outside the dc workspace"
    assert not bool((out == sent).any()), "a dc element left unwritten"
    return out.clone()


@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_raw_calls_stay_inside_their_frames_and_repeat_their_bits(env, case_data, ci):
    c, d = CASES[ci], case_data[ci]
    ops, codes = env.ops, d["codes"]
    x_t, g_t, cen_t = _dev(d["xf"]), _dev(d["gf"]), _dev(d["cf"])
    dx = _raw_dx(env, c, codes, g_t, cen_t)
    assert torch.equal(dx, _raw_dx(env, c, codes, g_t, cen_t)), "dx: a second call gives other bits"
    assert torch.equal(dx.view(c["m"], c["kdim"]), _bits(ops.grouped_sparse_codebook_matmul_dx(g_t, codes, cen_t)))
    for f64 in (1, 0):
        dc = _raw_dc(env, c, codes, x_t, g_t, f64)
        assert torch.equal(dc, _raw_dc(env, c, codes, x_t, g_t, f64)), "dc: a second call gives other bits"
        want = ops.grouped_sparse_codebook_centroid_grad(x_t, g_t, codes, dtype=torch.float64 if f64 else torch.float32)
        assert torch.equal(dc, _bits(want).view(-1))


@pytest.mark.parametrize("m,kdim,ncols", ref.EMPTY)
def test_empty_shapes(env, m, kdim, ncols):
    ops = env.ops
    rng = np.random.RandomState(3)
    rows, k = 32, 16
    G = -(-kdim // rows)
    zs = torch.zeros(G, dtype=torch.uint8, device="cuda")
    lab_t = _dev_labels(rng.randint(0, k, size=(kdim, ncols)))
    codes = ops.pack_grouped_sparse_codes(lab_t, kdim, ncols, k, rows, zero_symbols=zs)
    cen_t = _dev(rng.standard_normal((max(G, 1), k)))
    g_t, x_t = _dev(rng.standard_normal((m, ncols))), _dev(rng.standard_normal((m, kdim)))
    dx = ops.grouped_sparse_codebook_matmul_dx(g_t, codes, cen_t)
    assert dx.shape == (m, kdim) and not bool(dx.any())             # NONE: empty; ZERO (ncols = 0): zero-filled
    for dt in (torch.float64, torch.float32):
        dc = ops.grouped_sparse_codebook_centroid_grad(x_t, g_t, codes, dtype=dt)
        assert dc.shape == (max(G, 1), k) and dc.dtype == dt and not bool(dc.any())


def test_m16_and_m17_agree_within_the_bound(env):
    """The stream kernel (m = 16) and the tiled one (m = 17, its first 16 rows) on the same data: each within the bound of the float64
    product, so within twice the bound of each other; dc of the two calls differs by the seventeenth row's exact terms only."""
    ops = env.ops
    c = dict(m=17, kdim=300, ncols=130, k=16, group_rows=32, off=0, pruned=False)
    lab, zs = ref.labels_of(c, 77)
    xf, gf, cf = ref.float_data(c, zs, 77)
    codes = ops.pack_grouped_sparse_codes(_dev_labels(lab), c["kdim"], c["ncols"], c["k"], 32, zero_symbols=torch.from_numpy(zs).cuda())
    cen_t = _dev(cf)
    a = ops.grouped_sparse_codebook_matmul_dx(_dev(gf[:16]), codes, cen_t).cpu().numpy().astype(np.float64)
    b = ops.grouped_sparse_codebook_matmul_dx(_dev(gf), codes, cen_t).cpu().numpy().astype(np.float64)
    r64, bound = ref.dx_bound(gf, lab, cf, zs, 32)
    assert np.all(np.abs(a - r64[:16]) <= bound[:16]) and np.all(np.abs(b - r64) <= bound)
    assert np.all(np.abs(a - b[:16]) <= 2 * bound[:16])


# ------------------------------------------------------------------ check 8: autograd
@pytest.mark.parametrize("ci", [0, 1, 4, 9, 10, 12], ids=[IDS[i] for i in (0, 1, 4, 9, 10, 12)])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_autograd_against_the_byte_grouped_layer(env, case_data, ci, relu):
    c, d = CASES[ci], case_data[ci]
    ops, rows = env.ops, c["group_rows"]
    rng = np.random.RandomState(40 + ci)
    for exact in (True, False):
        x, cen = (d["x"], d["cen"]) if exact else (d["xf"], d["cf"])
        if exact:   # integers small enough that y, its mask and every backward sum are exact in both forms
            bias, gy = rng.randint(-5, 6, size=c["ncols"]).astype(np.float32), np.clip(d["g"], -1, 1)
        else:
            bias, gy = rng.standard_normal(c["ncols"]).astype(np.float32), d["gf"]
        leaves = [[_dev(t).requires_grad_(True) for t in (x, cen, bias)] for _ in range(2)]
        (xs, cs, bs), (xb, cb, bb) = leaves
        ys = ops.grouped_sparse_codebook_linear(xs, d["codes"], cs, bias=bs, relu=relu)
        yb = ops.grouped_codebook_linear(xb, d["unpacked"], cb, c["kdim"], c["ncols"], rows, bias=bb, relu=relu)
        with torch.no_grad():   # under no_grad: grouped_sparse_codebook_matmul's bits
            assert torch.equal(_bits(ys), _bits(ops.grouped_sparse_codebook_linear(xs, d["codes"], cs, bias=bs, relu=relu)))
            assert torch.equal(_bits(ys), _bits(ops.grouped_sparse_codebook_matmul(xs, d["codes"], cs, bias=bs, relu=relu)))
        gy_t = _dev(gy)
        ys.backward(gy_t)
        g_t = torch.where(ys.detach() > 0, gy_t, torch.zeros((), device="cuda")) if relu else gy_t   # the fused ReLU masks g first
        assert torch.equal(_bits(xs.grad), _bits(ops.grouped_sparse_codebook_matmul_dx(g_t, d["codes"], cs.detach())))
        assert torch.equal(_bits(cs.grad), _bits(ops.grouped_sparse_codebook_centroid_grad(xs.detach(), g_t, d["codes"], dtype=torch.float32)))
        assert torch.equal(_bits(bs.grad), _bits(g_t.sum(0, dtype=torch.float32)))
        if relu and not exact:
            continue   # (the two forwards differ in their last bits, so the masks can differ where y is about 0: compared on exact data)
        if exact:
            assert torch.equal(ys, yb)
        yb.backward(gy_t)
        # the same g reaches both backward passes (exact data: the same y and mask; no ReLU: g is gy): the centres' gradient bit for bit
        assert torch.equal(_bits(cs.grad), _bits(cb.grad)) and torch.equal(_bits(bs.grad), _bits(bb.grad))
        if exact:
            assert torch.equal(xs.grad, xb.grad)
        else:
            r64, bound = ref.dx_bound(gy, d["lab"], cen, d["zs"], rows)
            assert np.all(np.abs(xs.grad.cpu().numpy().astype(np.float64) - r64) <= bound)


def test_the_ops_refuse_half_inputs_wrong_kinds_and_shapes(env, case_data):
    ops = env.ops
    c, d = CASES[0], case_data[0]
    x_t, g_t, cen_t = _dev(d["xf"]), _dev(d["gf"]), _dev(d["cf"])
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="float32 activations"):
            ops.grouped_sparse_codebook_linear(x_t.to(dt), d["codes"], cen_t)
        with pytest.raises(TypeError, match="float32 activations"):
            ops.grouped_sparse_codebook_matmul_dx(g_t.to(dt), d["codes"], cen_t)
        with pytest.raises(TypeError, match="float32 activations"):
            ops.grouped_sparse_codebook_centroid_grad(x_t.to(dt), g_t.to(dt), d["codes"])
    with pytest.raises(RuntimeError, match="inference only"):      # the inference op keeps raising under autograd
        ops.grouped_sparse_codebook_matmul(x_t.clone().requires_grad_(True), d["codes"], cen_t)
    with pytest.raises(TypeError, match="GroupedSparseCodes"):
        ops.grouped_sparse_codebook_matmul_dx(g_t, d["unpacked"], cen_t)
    with pytest.raises(ValueError, match="centers must have shape"):
        ops.grouped_sparse_codebook_matmul_dx(g_t, d["codes"], cen_t[:1])
    with pytest.raises(ValueError, match="g must have shape"):
        ops.grouped_sparse_codebook_matmul_dx(g_t[:, :-1].contiguous(), d["codes"], cen_t)
    with pytest.raises(ValueError, match="x must have shape"):
        ops.grouped_sparse_codebook_centroid_grad(x_t[:, :-1].contiguous(), g_t, d["codes"])
    with pytest.raises(TypeError, match="dtype must be"):
        ops.grouped_sparse_codebook_centroid_grad(x_t, g_t, d["codes"], dtype=torch.float16)
    dx3 = ops.grouped_sparse_codebook_matmul_dx(g_t.view(1, c["m"], c["ncols"]), d["codes"], cen_t)     # leading dimensions are kept
    assert dx3.shape == (1, c["m"], c["kdim"])


def test_forward_and_backward_read_nothing_back(env, case_data):
    ops = env.ops
    for ci in (4, 11):   # m = 16 (stream) and m = 17 (tiled, dx split)
        c, d = CASES[ci], case_data[ci]
        xt, ct = _dev(d["xf"]).requires_grad_(True), _dev(d["cf"]).requires_grad_(True)
        bt = torch.zeros(c["ncols"], device="cuda", requires_grad=True)
        gy = torch.ones(c["m"], c["ncols"], device="cuda")
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for relu in (False, True):
                ops.grouped_sparse_codebook_linear(xt, d["codes"], ct, bias=bt, relu=relu).backward(gy)
        finally:
            torch.cuda.set_sync_debug_mode(0)


# ------------------------------------------------------------------ check 9: no byte-per-weight tensor in the backward
def test_backward_peak_allocation_stays_below_a_byte_per_weight(env):
    ops = env.ops
    kdim = ncols = 2048
    k, rows, m = 16, 128, 1
    keep = torch.rand(kdim * ncols, device="cuda") < 0.1
    labels = torch.where(keep, torch.randint(1, k, (kdim * ncols,), device="cuda"), torch.zeros((), dtype=torch.int64, device="cuda")).to(torch.uint8)
    del keep
    codes = ops.pack_grouped_sparse_codes(labels, kdim, ncols, k, rows, zero_symbols=torch.zeros(kdim // rows, dtype=torch.uint8, device="cuda"))
    del labels
    assert codes.nbytes() < 0.35 * kdim * ncols
    ct = (torch.randn(kdim // rows, k, device="cuda") * 0.1).requires_grad_(True)
    xt = torch.randn(m, kdim, device="cuda").requires_grad_(True)
    y = ops.grouped_sparse_codebook_linear(xt, codes, ct)
    gy = torch.randn_like(y)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y.backward(gy)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    print(f"backward peak over the baseline: {growth} bytes; a byte per weight: {kdim * ncols}")
    assert growth < kdim * ncols
    assert xt.grad.shape == (m, kdim) and ct.grad.shape == (kdim // rows, k)


# ------------------------------------------------------------------ check 10: the layer, the network function, the trainer
class _Net(torch.nn.Module):
    def __init__(self, **layers):
        super().__init__()
        self._names = list(layers)
        for name, layer in layers.items():
            setattr(self, name, layer)

    def get_config(self):
        return {name: getattr(self, name) for name in self._names}

    def forward(self, x):
        for name in self._names:
            x = getattr(self, name)(x)
        return x


class _Dense:
    """A stand-in with the attributes the constructors read (hashable: a key of models_by_layer)."""

    def __init__(self, **attrs):
        self.__dict__.update(attrs)


def _grouped_layer(compressed, rng, kdim, ncols, k, rows, density, activation):
    zs = (1 + 2 * np.arange(-(-kdim // rows))) % k
    lab = np.concatenate([sparse_ref.labels_at_density(rng, min(kdim, (q + 1) * rows) - q * rows, ncols, k, density, int(z))
                          for q, z in enumerate(zs)], axis=0)
    cen = (rng.randint(-8, 9, size=(len(zs), k)) / 4.0).astype(np.float32)
    bias = rng.randint(-5, 6, size=ncols).astype(np.float32)
    return compressed.GroupedCompressedDense.from_codes(kdim, ncols, rows, _dev_labels(lab, 1), _dev(cen), _dev(bias), activation), lab, zs


def test_the_layer_and_its_four_constructors(env):
    from neural_network_compression_amd import compressed

    ops = env.ops
    rng = np.random.RandomState(21)
    byte, lab, zs = _grouped_layer(compressed, rng, 96, 64, 16, 32, 0.1, torch.relu)
    cls = compressed.TrainableGroupedSparseCompressedDense
    twin = compressed.TrainableGroupedCompressedDense.from_grouped(byte)
    sparse = compressed.GroupedSparseCompressedDense.from_grouped(byte)
    dense = types.SimpleNamespace(kernel=torch.zeros(96, 64, device="cuda"), bias=byte.bias, activation=torch.relu)
    model = types.SimpleNamespace(cluster_centers_=byte.centers.cpu().numpy(), group_rows=32, labels_compact_=byte.labels)
    a, b = cls.from_grouped(byte), cls.from_grouped_sparse(sparse)
    cc = cls.from_codes(96, 64, 32, byte.labels, byte.centers, bias=byte.bias, activation=torch.relu)
    dd = cls.from_dense(dense, model)
    assert b.packed.data_ptr() == sparse.packed.data_ptr()                   # the same buffer: nothing repacked
    nnz = int(fwd.keep_mask(lab, zs, 32).sum())
    x = _dev(rng.randint(-3, 4, size=(5, 96)))
    for layer in (a, b, cc, dd):
        assert isinstance(layer, compressed._TrainableCentres) and not hasattr(layer, "labels")
        assert isinstance(layer.centers, torch.nn.Parameter) and layer.centers.shape == layer.counts.shape == (3, 16)
        assert torch.equal(layer.packed, a.packed) and torch.equal(layer.zero_symbols, a.zero_symbols) and layer.nnz == nnz
        assert np.array_equal(layer.zero_symbols.cpu().numpy(), zs)
        assert torch.equal(layer.counts, twin.counts) and int(layer.counts.sum()) == 96 * 64
        assert torch.equal(_bits(layer.kernel_sq_sum()), _bits(twin.kernel_sq_sum()))          # the byte grouped layer's, bit for bit
        assert all(buf.numel() < 96 * 64 for _, buf in layer.named_buffers())                  # no byte-per-weight buffer
        parts = sparse_ref.layout(96, 64, 1, nnz)["bytes"] + 3 + 4 * 3 * 16 + 4 * 64
        assert layer.nbytes() == parts == compressed.compressed_nbytes(layer) == sparse.nbytes()
        assert layer.get_weights() == [] and torch.equal(layer.codes.to_dense(), byte.labels)
        with torch.no_grad():
            assert torch.equal(layer(x), sparse(x)) and torch.equal(layer(x), byte(x))          # exact data: the byte layer's output too
        with pytest.raises(TypeError, match="float32 activations"):
            layer(x.to(torch.bfloat16))
    # a step through the layer: the gradients of the ops
    y = a(x.clone().requires_grad_(True))
    (y.sum() + 0.01 * a.kernel_sq_sum()).backward()
    assert a.centers.grad is not None and a.centers.grad.shape == (3, 16)
    # the state dict round trip keeps the layer
    again = cls.from_grouped(byte)
    again.load_state_dict(a.state_dict())
    with torch.no_grad():
        assert torch.equal(_bits(again(x)), _bits(a(x)))


def test_compress_network_trainable_grouped_picks_forms_by_bytes(env):
    from neural_network_compression_amd import compressed

    rng = np.random.RandomState(33)
    specs = dict(a=(96, 64, 16, 0.1),     # pruned: sparse < packed < byte
                 b=(64, 64, 16, 1.0),     # dense: packed < byte < sparse
                 c=(64, 16, 16, 1.0),     # 16-byte packed rows of 16 columns: byte == packed < sparse
                 d=(96, 64, 17, 0.1))     # K = 17 and pruned: no packed form; sparse < byte
    layers, models = {}, {}
    for name, (kdim, ncols, k, density) in specs.items():
        byte, _, _ = _grouped_layer(compressed, rng, kdim, ncols, k, 32, density, None)
        dense = _Dense(kernel=torch.zeros(kdim, ncols, device="cuda"), bias=byte.bias, activation=None)
        layers[name] = dense
        models[dense] = [types.SimpleNamespace(cluster_centers_=byte.centers.cpu().numpy(), group_rows=32, labels_compact_=byte.labels), None]
    net = _Dense(get_config=lambda: layers, **layers)
    B, Pk, Sp = (compressed.TrainableGroupedCompressedDense, compressed.TrainableGroupedPackedCompressedDense,
                 compressed.TrainableGroupedSparseCompressedDense)

    def kinds(**kw):
        out = compressed.compress_network_trainable_grouped(net, models, **kw)
        return [type(getattr(out, n)) for n in "abcd"], out

    assert kinds()[0] == kinds(sparse=False)[0] == [B, B, B, B]
    assert kinds(sparse=True)[0] == [Sp, Sp, Sp, Sp]
    assert kinds(sparse="auto")[0] == [Sp, B, B, Sp]
    got, out = kinds(sparse="auto", packed="auto")
    assert got == [Sp, Pk, B, Sp]                                  # on equal bytes the order is byte, packed, sparse
    for n in "abcd":
        cands = [B.from_dense(layers[n], *models[layers[n]])]
        if specs[n][2] <= 16:
            cands.append(Pk.from_dense(layers[n], *models[layers[n]]))
        cands.append(Sp.from_dense(layers[n], *models[layers[n]]))
        best = min(cands, key=lambda l: l.nbytes())                # min keeps the first of equals
        assert type(getattr(out, n)) is type(best) and getattr(out, n).nbytes() == best.nbytes(), n
    assert kinds(sparse="auto", packed=True)[0] == [Sp, Pk, Pk, Sp]   # packed=True: no byte candidate where K <= 16
    assert kinds(sparse=True, packed="auto")[0] == [Sp, Pk, Pk, Sp]   # sparse=True: no byte candidate anywhere
    for bad in (None, "yes", 2):
        with pytest.raises(ValueError, match="sparse"):
            kinds(sparse=bad)
    with pytest.raises(ValueError, match="half_inputs"):
        kinds(sparse=True, half_inputs=True)
    with pytest.raises(NotImplementedError, match="a"):            # the older door keeps refusing grouped layers
        compressed.compress_network(net, models, sparse=True)


def test_a_step_through_two_layers_on_exact_data_is_the_byte_forms_bit_for_bit(env):
    """The issue's first condition where it can hold.  Two stacked trainable layers (96 -> 64 with ReLU, 64 -> 10), quarter-integer
    centres and integer bias (_grouped_layer), integer x in [-3, 3], the gradient of the output integers in [-1, 1], the trainers' L2
    term on the centres.  Every forward sum is exact (layer 1: terms in quarter-units, their magnitudes below 96 * 3 * (4 + 2) * 4;
    layer 2: sixteenth-units, below 64 * 600 * 6 * 16 < 2^24), so both forms give the same y and the same ReLU mask; dx of the second
    layer (|.| <= 10 * 6) is exact too, so the first layer sees the same g in both forms; dc is the same function bit for bit.  So
    one step, c - lr * grad, ends with the byte form's centres bit for bit in both layers, the first one's through the second one's dx."""
    from neural_network_compression_amd import compressed

    rng = np.random.RandomState(52)
    b1, _, _ = _grouped_layer(compressed, rng, 96, 64, 16, 32, 0.1, torch.relu)
    b2, _, _ = _grouped_layer(compressed, rng, 64, 10, 16, 32, 0.3, None)
    x = _dev(rng.randint(-3, 4, size=(5, 96)))
    gy = _dev(rng.randint(-1, 2, size=(5, 10)))
    tuned = {}
    for form, cls in (("byte", compressed.TrainableGroupedCompressedDense), ("sparse", compressed.TrainableGroupedSparseCompressedDense)):
        l1, l2 = cls.from_grouped(b1), cls.from_grouped(b2)
        y = l2(l1(x))
        ((y * gy).sum() + 0.01 * (l1.kernel_sq_sum() + l2.kernel_sq_sum()) / 2).backward()
        with torch.no_grad():
            tuned[form] = [(l.centers - 1e-2 * l.centers.grad).clone() for l in (l1, l2)] + [y.detach().clone()]
        assert bool(l1.centers.grad.any()) and bool(l2.centers.grad.any())
    for a, b in zip(tuned["sparse"], tuned["byte"]):
        assert torch.equal(_bits(a), _bits(b))


GR, LR = 32, 1e-2
DENSE = ("dense1", "dense2", "out")


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


def test_one_epoch_of_fine_tune_grouped_sparse_on_a_pruned_lenet(env):
    """One batch of 512 on a pruned LeNet-300-100 quantized with group_rows = 32.  The loss depends on every layer's forward, and the
    sparse forward sums in another order than the byte form's, so the tuned centres are not the byte form's bit for bit; what holds
    bit for bit is the step itself: the tuned centres are c - lr * (the centres' gradient of the same trainable network), the centroid
    gradient being ops.grouped_sparse_codebook_centroid_grad's.  Against the byte form's fine_tune_grouped() the centres agree within
    the tolerance the byte and packed fine-tune tests derive for the float64 step, which bounds chain lengths (784 + 300 + 100 + 16
    operations), not summation orders.  That tolerance is taken unchanged.  It applies to the sparse form because the test's network
    has c_z == 0 exactly in every group: every group's skipped symbol is its pruned cluster, whose centre the test sets to 0 (the fit leaves a
    residue of about 1e-8 there) before either run.  Then d = c, there is no rank-1 term, and every sparse sum is the
    byte form's sum with its zero terms left out: no chain is longer.  Each run is within the tolerance of the float64 step, so the
    two are within its double of each other (the triangle inequality).  The issue's first condition, the byte form's centres bit for
    bit, is held where it can hold, on exact data, by test_a_step_through_two_layers_on_exact_data_is_the_byte_forms_bit_for_bit."""
    from neural_network_compression_amd import compressed
    from neural_network_compression_amd.common import trainer as tr

    ops = env.ops
    rng = np.random.RandomState(1)
    x = rng.rand(512, 784).astype(np.float32)
    y = np.eye(10, dtype=np.float32)[rng.randint(0, 10, size=512)]
    data, test = tr.LeNetDataset(x, y), tr.LeNetDataset(x[:128], y[:128].argmax(1))
    runs = {}
    for form in ("sparse", "byte"):
        t = _trainer()
        t._prune_parameters(True)
        t.quantize(test, False, 4, "linear", group_rows=GR)
        models, cfg = t.quantized_models_by_layer, t.neural_network.get_config()
        for n in DENSE:   # every group's most frequent index (the pruned cluster, its fitted centre a residue of 1e-8) gets the
            wm = models[cfg[n]][0]   # centre 0 exactly, in both runs: the network under test is the one these models describe
            kin, kout = cfg[n].kernel.shape
            lab = wm.labels_compact_.cpu().numpy().reshape(kin, kout)
            for q, gm in enumerate(wm.models):
                z = int(np.argmax(np.bincount(lab[q * GR: (q + 1) * GR].ravel(), minlength=16)))
                wm.cluster_centers_[q, z] = 0.0
                gm.cluster_centers_[z] = 0.0
        start = {n: models[cfg[n]][0].cluster_centers_.copy() for n in DENSE}
        labels = {n: models[cfg[n]][0].labels_compact_.cpu().numpy().astype(np.int64) for n in DENSE}
        bias0 = {n: cfg[n].bias.detach().double().cpu().clone() for n in DENSE}
        kw = dict(sparse=True) if form == "sparse" else {}
        manual = compressed.compress_network_trainable_grouped(t.neural_network, models, **kw)
        params = [p for n in DENSE for p in (getattr(manual, n).centers, getattr(manual, n).bias_centers) if p is not None]
        for p in manual.parameters():
            p.requires_grad_(False)
        for p in params:
            p.requires_grad_(True)
        torch.manual_seed(11)                                          # the trainer's one batch: the 512 rows in its shuffled order
        xb, yb = next(iter(tr._batches(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())))
        t._get_error(xb, yb, manual).backward()
        step = {n: (getattr(manual, n).centers.detach() - LR * getattr(manual, n).centers.grad) for n in DENSE}
        built = []
        real = compressed.compress_network_trainable_grouped

        def spy(*a, **k):
            built.append((real(*a, **k), k))
            return built[-1][0]

        compressed.compress_network_trainable_grouped = spy
        torch.manual_seed(11)
        try:
            acc = t.fine_tune_grouped(data, test, epochs=1, learning_rate=LR, **kw)
        finally:
            compressed.compress_network_trainable_grouped = real
        assert len(acc) == 1 and 0.0 <= acc[0] <= 1.0
        assert built[0][1] == (dict(packed=False, sparse=True) if form == "sparse" else dict(packed=False))
        net = built[0][0]
        after = t.compressed_network()
        for n in DENSE:
            layer = getattr(net, n)
            want = compressed.TrainableGroupedSparseCompressedDense if form == "sparse" else compressed.TrainableGroupedCompressedDense
            assert type(layer) is want, n
            tuned = layer.centers.detach()
            assert torch.equal(_bits(tuned), _bits(step[n])), (form, n)                      # the step, bit for bit
            assert not np.array_equal(tuned.cpu().numpy(), start[n])                        # the centres moved
            assert np.array_equal(models[cfg[n]][0].cluster_centers_, tuned.cpu().numpy())  # the write-back of the tuned (G, K)
            assert torch.equal(getattr(after, n).centers, tuned), n                         # visible in compressed_network()
        if form == "sparse":
            for n in DENSE:   # every group skips its pruned cluster: c_z == 0 exactly
                layer = getattr(net, n)
                c0 = torch.from_numpy(np.ascontiguousarray(start[n], dtype=np.float32)).cuda()
                cz = torch.gather(c0, 1, layer.zero_symbols.long().view(-1, 1))
                assert not bool(cz.any()), n
                assert layer.nnz < layer.kdim * layer.ncols, n        # pruned: some weights are skipped
        runs[form] = dict(start=start, labels=labels, bias=bias0, tuned={n: getattr(net, n).centers.detach().cpu().numpy().astype(np.float64) for n in DENSE},
                          kernels={n: cfg[n].kernel.shape for n in DENSE}, t=t)
    # the float64 step of the decoded network, and the tolerance of the byte / packed fine-tune tests
    s = runs["byte"]
    assert all(np.array_equal(runs["sparse"]["start"][n], s["start"][n]) and np.array_equal(runs["sparse"]["labels"][n], s["labels"][n]) for n in DENSE)
    ws, bs = [], []
    for n in DENSE:
        kin, kout = s["kernels"][n]
        w = np.take_along_axis(np.repeat(s["start"][n].astype(np.float64), GR, axis=0)[:kin], s["labels"][n].reshape(kin, kout), axis=1)
        ws.append(torch.from_numpy(w).requires_grad_(True))
    bs = [s["bias"][n] for n in DENSE]
    a, xs, zs = torch.from_numpy(x).double(), [], []
    for i, (w, b) in enumerate(zip(ws, bs)):
        xs.append(a)
        z = a @ w + b
        z.retain_grad()
        zs.append(z)
        a = torch.relu(z) if i < 2 else z
    loss = torch.nn.functional.binary_cross_entropy_with_logits(a, torch.from_numpy(y).double()) + 0.01 * sum((w ** 2).sum() / 2 for w in ws)
    loss.backward()
    u = cbgrad_ref.U
    for i, n in enumerate(DENSE):
        kin, kout = s["kernels"][n]
        case = dict(m=512, kdim=kin, ncols=kout, k=16, group_rows=GR, off=0)
        lab = s["labels"][n].reshape(kin, kout)
        x64, g64, dw = xs[i].detach().numpy(), zs[i].grad.numpy(), ws[i].grad.numpy()
        G = grouped_grad_ref.groups_of(case)
        rows_of = [grouped_grad_ref.group_rows_of(case, q) for q in range(G)]
        dc64 = np.stack([cbgrad_ref.bin64(dw[r], lab[r], 16) for r in rows_of])
        tl = ops.cbsp_grouped_dc_plan(512, kin, kout, 16, GR, env.cus)["terms_log2"]
        S, flag = ops.cbgrad_shift(512, np.abs(x64).max(), np.abs(g64).max(), tl)
        assert flag == ops.CBGRAD_OK
        bound = grouped_grad_ref.dc_bound(case, x64.astype(np.float32), g64.astype(np.float32), lab, S - 1, f32_out=True)
        mag = np.stack([cbgrad_ref.bin64(cbgrad_ref.dw64(np.abs(x64[:, r]), np.abs(g64)), lab[r], 16) for r in rows_of])
        counts = np.stack([np.bincount(lab[r].ravel(), minlength=16) for r in rows_of])
        l2 = 0.01 * counts * np.abs(s["start"][n].astype(np.float64))
        tol = LR * (bound + 2 * 1200 * u * mag + 8 * u * l2 + 4 * u * np.abs(dc64))
        want = s["start"][n].astype(np.float64) - LR * dc64
        tol = tol + 2 * u * np.abs(want)
        for form in ("sparse", "byte"):
            err = np.abs(runs[form]["tuned"][n] - want)
            print(f"{n} {form}: max |got - want| {err.max():.3e}, its tolerance {tol[np.unravel_index(err.argmax(), err.shape)]:.3e}")
            assert np.all(err <= tol), (n, form)
        assert np.all(np.abs(runs["sparse"]["tuned"][n] - runs["byte"]["tuned"][n]) <= 2 * tol), n
