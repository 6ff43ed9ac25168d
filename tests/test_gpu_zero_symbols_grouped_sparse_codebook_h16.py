"""The group-wise codebook layer run from the bitmap-sparse form of its indices on bf16 / fp16 activations (nnc_cbsp_grouped_h16,
csrc/nnc_cbsp_grouped_h16.hip) through ops.grouped_sparse_codebook_matmul(half_inputs=True),
GroupedSparseCompressedDense(half_inputs=True), sparsify_grouped_layers and smallest_grouped_layers (run with -m gpu).  No tolerance
anywhere: every comparison is bit for bit, against
  - m > 16: ops.grouped_codebook_matmul on the unpacked labels and the same half x (the MFMA tile, k_cbspg_mfma), also with Inf and
    NaN in x;
  - m <= 16: ops.grouped_sparse_codebook_matmul on x.float() and centers.to(dtype).float() (the stream path), the half output one
    rounding of it;
  - the float64 formula on exact data in every regime, W_h itself through x = I, and ops.sparse_codebook_matmul with one group."""
import ctypes
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import grouped_ref, h16_ref, sparse_ref  # noqa: E402
from tests.helpers import grouped_sparse_h16_ref as href  # noqa: E402
from tests.helpers import grouped_sparse_ref as ref  # noqa: E402
from tests.helpers.cbmm_ref import relu_like_torch  # noqa: E402

CASES = href.CASES
IDS = [href.case_id(c) for c in CASES]
DTYPES = href.DTYPES
BIG = [i for i, c in enumerate(CASES) if c["m"] > 16]
SMALL = [i for i, c in enumerate(CASES) if c["m"] <= 16]
TINY = {"fp16": 1e-9, "bf16": 1e-41}   # non-zero in float32, 0 once rounded to the dtype (fp16: below 2^-25; bf16: below 2^-134)


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native as nat
    from neural_network_compression_amd import ops

    _, cus = ops.device_info()
    assert cus >= 1
    return types.SimpleNamespace(ops=ops, nat=nat, cus=cus)


def _dev(host):
    return torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).cuda()


def _half(host, dtype, view=False, fill=0.0):
    """host float32 values (representable in ``dtype``) -> device tensor of the dtype; ``view``: as buf[1:] of a longer buffer filled
    with ``fill`` on both sides (2-byte aligned and no further)."""
    t = torch.from_numpy(np.ascontiguousarray(host, dtype=np.float32)).cuda().to(h16_ref.torch_dtype(dtype))
    if not view:
        return t
    buf = torch.full((t.numel() + 9,), fill, dtype=t.dtype, device="cuda")
    buf[1: 1 + t.numel()] = t.reshape(-1)
    out = buf[1: 1 + t.numel()].view(t.shape)
    assert out.data_ptr() % 16 == 2
    return out


def _dev_labels(lab, off=0):
    host = np.ascontiguousarray(np.asarray(lab).ravel().astype(np.uint8))
    buf = torch.zeros(off + host.size + 16, dtype=torch.uint8, device="cuda")
    buf[off: off + host.size] = torch.from_numpy(host).cuda()
    return buf[off: off + host.size]


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def case_data(env):
    """Per case, made once and left unchanged: the labels and their packed form on the device, exact and float data on the host."""
    out = []
    for ci, c in enumerate(CASES):
        lab, zs, x, cen, bias = ref.exact_data(c, 300 + ci, ci)
        xf, cf, bf = ref.float_data(c, zs, 300 + ci)
        zs_t = torch.from_numpy(zs).cuda()
        codes = env.ops.pack_grouped_sparse_codes(_dev_labels(lab, c["off"]), c["kdim"], c["ncols"], c["k"], c["group_rows"], zero_symbols=zs_t)
        assert codes.buf.numel() == sparse_ref.layout(c["kdim"], c["ncols"], 1, codes.nnz)["bytes"]   # the symbols end with their tensor
        out.append(dict(lab=lab, zs=zs, x=x, cen=cen, bias=bias, xf=xf, cf=cf, bf=bf, codes=codes, dense=codes.to_dense()))
    return out


def _op(env, x_t, d, cen_t, bias_t=None, relu=False, out_dtype=None):
    with torch.no_grad():
        return env.ops.grouped_sparse_codebook_matmul(x_t, d["codes"], cen_t, bias=bias_t, relu=relu, out_dtype=out_dtype, half_inputs=True)


def test_the_case_list_reaches_every_regime_and_group_walk_at_this_device(env, case_data):
    hit, feats, kinds = set(), set(), {False: set(), True: set()}
    for c, d in zip(CASES, case_data):
        for dtype in DTYPES:
            plan = env.ops.cbsp_grouped_h16_plan(h16_ref.torch_dtype(dtype), c["m"], c["kdim"], c["ncols"], c["k"], c["group_rows"], env.cus)
            hit.add(href.regime_of(plan, dtype))
            feats |= href.features_of(c, plan)
        kept = ref.keep_mask(d["lab"], d["zs"], c["group_rows"])
        for g, z in enumerate(d["zs"]):
            rows = slice(g * c["group_rows"], (g + 1) * c["group_rows"])
            share = kept[rows].mean()
            kinds[c["m"] > 16] |= {"pruned"} if share == 0 else ({"full"} if share == 1 else set())
            kinds[c["m"] > 16] |= {"z past K"} if z >= c["k"] else set()
            kinds[c["m"] > 16] |= {"stored label past K"} if (d["lab"][rows][kept[rows]] >= c["k"]).any() else set()
    assert hit == href.required_regimes(), sorted(href.required_regimes() ^ hit)
    assert feats >= href.required_features(), sorted(href.required_features() - feats)
    assert kinds[False] == kinds[True] == {"pruned", "full", "z past K", "stored label past K"}   # point 7, on both paths


# ------------------------------------------------------------------ 1. m > 16: the MFMA path against the byte form
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci", BIG, ids=[IDS[i] for i in BIG])
def test_above_16_rows_is_the_grouped_byte_form_on_the_unpacked_labels_bit_for_bit(env, case_data, ci, dtype):
    c, d = CASES[ci], case_data[ci]
    cen_t = _dev(d["cf"])
    bias_t = None if d["bf"] is None else _dev(d["bf"])
    x = h16_ref.round_to(d["xf"], dtype).reshape(d["xf"].shape)
    bad = x.copy()
    rng = np.random.RandomState(ci)
    for v in (np.inf, -np.inf, np.nan):
        bad[rng.randint(c["m"]), rng.randint(c["kdim"])] = v
    skipped = np.argwhere(~ref.keep_mask(d["lab"], d["zs"], c["group_rows"]))
    if len(skipped):   # (a case whose only group has density 1.0 has none)
        bad[c["m"] - 1, skipped[len(skipped) // 2][0]] = np.inf   # an Inf at a skipped position: an entry of W_h here, as in the byte form
    for values in (x, bad):
        x_t = _half(values, dtype, c["x_view"])
        for relu in (False, True):
            for out_dtype in (None, torch.float32):
                y = _op(env, x_t, d, cen_t, bias_t, relu, out_dtype)
                with torch.no_grad():
                    want = env.ops.grouped_codebook_matmul(x_t, d["dense"], cen_t, c["kdim"], c["ncols"], c["group_rows"], bias=bias_t, relu=relu,
                                                           out_dtype=out_dtype)
                assert y.dtype == (x_t.dtype if out_dtype is None else torch.float32) and y.shape == (c["m"], c["ncols"])
                assert _same(y, want), (relu, out_dtype)
        if values is bad:
            assert torch.isnan(want).any()   # the NaN in x reaches its whole row, through ReLU too


# ------------------------------------------------------------------ 2. m <= 16: the stream path against the float32 product
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci", SMALL, ids=[IDS[i] for i in SMALL])
def test_up_to_16_rows_is_the_float32_product_of_the_widened_x_and_the_rounded_centres(env, case_data, ci, dtype):
    c, d = CASES[ci], case_data[ci]
    tdt = h16_ref.torch_dtype(dtype)
    cen_t = _dev(d["cf"])
    cen_r = cen_t.to(tdt).float()
    bias_t = None if d["bf"] is None else _dev(d["bf"])
    x_t = _half(h16_ref.round_to(d["xf"], dtype).reshape(d["xf"].shape), dtype, c["x_view"])
    for relu in (False, True):
        with torch.no_grad():
            want = env.ops.grouped_sparse_codebook_matmul(x_t.float(), d["codes"], cen_r, bias=bias_t, relu=relu)
        y32 = _op(env, x_t, d, cen_t, bias_t, relu, torch.float32)
        assert _same(y32, want), relu
        assert _same(_op(env, x_t, d, cen_t, bias_t, relu), want.to(tdt)), relu


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,kdim", [(1, 128), (16, 128), (3, 1000)], ids=["m1", "m16", "m3-split"])
def test_an_inf_at_a_skipped_position_of_a_group_whose_rounded_cz_is_zero_leaves_y_finite(env, m, kdim, dtype):
    """Group 1 has c_z == 0 exactly, group 2 a c_z that is non-zero in float32 and 0 once rounded to the dtype: the skipped weights of
    both are absent on the stream path and neither adds to t.  The other groups keep their rank-1 terms."""
    ops, tdt = env.ops, h16_ref.torch_dtype(dtype)
    rng = np.random.RandomState(m + kdim)
    ncols, k, rows = 70, 16, 32
    groups = -(-kdim // rows)
    zs = ((3 + 2 * np.arange(groups)) % k).astype(np.uint8)
    lab = np.concatenate([sparse_ref.labels_at_density(rng, min(kdim, (g + 1) * rows) - g * rows, ncols, k, 0.3, int(z)) for g, z in enumerate(zs)], axis=0)
    lab[40], lab[70] = zs[1], zs[2]                              # rows 40 (group 1) and 70 (group 2) are skipped entirely
    cen = (rng.standard_normal((groups, k)) + 2.0).astype(np.float32)
    cen[1, zs[1]], cen[2, zs[2]] = 0.0, TINY[dtype]
    assert cen[2, zs[2]] != 0 and h16_ref.round_to(cen[2, zs[2]: zs[2] + 1], dtype)[0] == 0
    x = h16_ref.round_to(rng.standard_normal((m, kdim)), dtype).reshape(m, kdim)
    x[m - 1, 40], x[0, 70] = np.inf, -np.inf
    codes = ops.pack_grouped_sparse_codes(_dev_labels(lab), kdim, ncols, k, rows, zero_symbols=torch.from_numpy(zs).cuda())
    d = dict(codes=codes)
    x_t, cen_t = _half(x, dtype), _dev(cen)
    y = _op(env, x_t, d, cen_t, out_dtype=torch.float32)
    assert torch.isfinite(y).all()
    with torch.no_grad():
        assert _same(y, ops.grouped_sparse_codebook_matmul(x_t.float(), codes, cen_t.to(tdt).float()))
    assert torch.isfinite(_op(env, x_t, d, cen_t)).all()
    # the departure: from 17 rows on a skipped weight is an entry of W_h, and the same Inf meets its 0
    x17 = np.concatenate([x[:1]] * 17, axis=0)
    assert torch.isnan(_op(env, _half(x17, dtype), d, cen_t)).all()


# ------------------------------------------------------------------ 3. exact data in every regime
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_exact_data_is_the_float64_formula_in_every_regime(env, case_data, ci, dtype):
    c, d = CASES[ci], case_data[ci]
    tdt = h16_ref.torch_dtype(dtype)
    cen = grouped_ref.round_centres(d["cen"], dtype)             # rounded first: still on the quarter grid
    assert np.array_equal(cen * 4, np.round(cen * 4))
    assert 4.0 * ref._magnitude(d["x"], d["lab"], cen, d["zs"], c["group_rows"], d["bias"]).max() < 2.0 ** 24   # every partial sum is exact
    want = ref.formula64(d["x"], d["lab"], cen, d["zs"], c["group_rows"], d["bias"])
    assert np.array_equal(want, grouped_ref.reference(d["x"], grouped_ref.weights(cen, d["lab"], c["kdim"], c["ncols"], c["group_rows"]), d["bias"]))
    x_t, cen_t = _half(d["x"], dtype, c["x_view"]), _dev(d["cen"])
    bias_t = None if d["bias"] is None else _dev(d["bias"])
    for relu in (False, True):
        w64 = relu_like_torch(want) if relu else want
        y32 = _op(env, x_t, d, cen_t, bias_t, relu, torch.float32)
        got = y32.cpu().numpy()
        assert np.array_equal(got.astype(np.float64), w64), (relu, float(np.abs(got - w64).max()))
        yh = _op(env, x_t, d, cen_t, bias_t, relu)
        assert _same(yh, torch.from_numpy(w64.astype(np.float32)).to(tdt).cuda()), relu
        assert _same(_op(env, x_t, d, cen_t, bias_t, relu, torch.float32), y32)   # the same call, the same bits


# ------------------------------------------------------------------ 4. the decode and the lane maps: x = I gives W_h itself
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("view", [False, True], ids=["aligned-x", "x-at-buf1"])
def test_the_identity_reads_w_h_itself_with_every_groups_own_z_and_table(env, dtype, view):
    """m = kdim = 112, four groups of 32 rows (a short last one), 130 columns: three segments, the last with two columns.  A different
    z in every group (group 2 skips a byte that names no centre: 0) and centres offset by 64 g, so a wrong table or a wrong group's z
    is off by 64 or more.  An aligned x takes the 16-byte fragment loads, buf[1:] the element loads."""
    c = ref._case(112, 112, 130, 16, bias=False)
    lab, zs, _, cen, _ = ref.exact_data(c, 41, 1)                # densities 0.3, 0.0 (c_z == 0), 1.0 (z past K), 0.05 by group
    assert len(set(zs.tolist())) == len(zs) == 4 and (zs >= 16).any()
    codes = env.ops.pack_grouped_sparse_codes(_dev_labels(lab, 1), 112, 130, 16, 32, zero_symbols=torch.from_numpy(zs).cuda())
    assert 0 < codes.nnz < 112 * 130
    x_t = _half(np.eye(112, dtype=np.float32), dtype, view)
    assert (x_t.data_ptr() % 16 == 0) != view
    w_h = grouped_ref.weights(cen, lab, 112, 130, 32, dtype)     # the skipped positions hold rn(c_{z_g}), or 0 for z_g >= K
    skipped = ~ref.keep_mask(lab, zs, 32)
    assert skipped[:32].any() and skipped[32:64].all() and not skipped[64:96].any() and skipped[96:].any()
    assert np.abs(w_h[:32][skipped[:32]]).max() > 0 and np.abs(w_h[96:][skipped[96:]]).min() >= 64   # rn(c_{z_0}), and rn(c_{z_3}) of group 3's table
    y = _op(env, x_t, dict(codes=codes), _dev(cen), out_dtype=torch.float32).cpu().numpy()
    assert np.array_equal(y, w_h), float(np.abs(y - w_h).max())
    yh = _op(env, x_t, dict(codes=codes), _dev(cen))
    assert _same(yh, torch.from_numpy(w_h).cuda().to(yh.dtype))


# ------------------------------------------------------------------ 5. one group against the ungrouped sparse product on half x
ONE_GROUP = [(17, 112, 130, 16), (17, 300, 50, 256), (130, 300, 129, 3),           # m > 16: direct, split, two tiles
             (1, 112, 70, 16), (4, 130, 64, 256), (16, 112, 130, 16),                # m <= 16 direct
             (2, 1500, 64, 3), (8, 2100, 50, 16)]                                   # m <= 16 split


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,kdim,ncols,k", ONE_GROUP, ids=[f"m{a}-kd{b}-n{c}-k{d}" for a, b, c, d in ONE_GROUP])
def test_one_group_is_the_ungrouped_sparse_product_on_half_x(env, m, kdim, ncols, k, dtype):
    ops = env.ops
    rng = np.random.RandomState(m * 1000 + kdim)
    z = 3 % k
    lab_t = _dev_labels(sparse_ref.labels_at_density(rng, kdim, ncols, k, 0.15, z), 1)
    rows = -(-kdim // 32) * 32 + 32 * (m % 2)                    # group_rows >= kdim: kdim rounded up, and beyond
    gcodes = ops.pack_grouped_sparse_codes(lab_t, kdim, ncols, k, rows, zero_symbols=torch.tensor([z], dtype=torch.uint8, device="cuda"))
    scodes = ops.pack_sparse_codes(lab_t, kdim, ncols, k, zero_symbol=z)
    x_t = _half(h16_ref.round_to(rng.standard_normal((m, kdim)), dtype).reshape(m, kdim), dtype)
    cen = rng.standard_normal(k).astype(np.float32)
    bias_t = _dev(rng.standard_normal(ncols))
    for cz_zero in ((True, False) if m > 16 else (True,)):       # m <= 16 with c_z != 0: the ungrouped kernel sums the row in another order
        cc = cen.copy()
        if cz_zero:
            cc[z] = 0.0
        cen_t = _dev(cc)
        for relu in (False, True):
            for out_dtype in (None, torch.float32):
                got = _op(env, x_t, dict(codes=gcodes), cen_t.view(1, k), bias_t, relu, out_dtype)
                with torch.no_grad():
                    want = ops.sparse_codebook_matmul(x_t, scodes, cen_t, bias=bias_t, relu=relu, out_dtype=out_dtype)
                assert _same(got, want), (cz_zero, relu, out_dtype)


# ------------------------------------------------------------------ 6. buffer edges and repeats
@pytest.mark.parametrize("dtype,y_half", [("bf16", True), ("fp16", False)], ids=["bf16-half-y", "fp16-float-y"])
@pytest.mark.parametrize("ci", [i for i, c in enumerate(CASES) if (c["m"], c["kdim"]) in ((1, 112), (8, 2100), (17, 112), (130, 300))],
                         ids=lambda i: IDS[i])
def test_nothing_is_written_outside_y_and_the_workspace_and_nothing_read_behind_x(env, case_data, ci, dtype, y_half):
    """The C entry point on buffers of its own: y and the workspace (of exactly the queried size) sit in frames of a sentinel that
    must survive, x sits between NaNs that must not reach y, and a second call gives the same bits."""
    c, d = CASES[ci], case_data[ci]
    nat, L = env.nat, env.nat.load()
    m, kdim, ncols, codes = c["m"], c["kdim"], c["ncols"], d["codes"]
    tdt = h16_ref.torch_dtype(dtype)
    code = href.DT_CODE[dtype]
    x_t = _half(d["x"], dtype, view=True, fill=float("nan"))
    cen_t = _dev(d["cen"])
    bias_t = None if d["bias"] is None else _dev(d["bias"])
    ydt = tdt if y_half else torch.float32
    frame, sentinel = 64, -12288.0   # exact in float32, bf16 and fp16
    ybuf = torch.full((frame + m * ncols + frame,), sentinel, dtype=ydt, device="cuda")
    ws_bytes = int(L.nnc_cbsp_grouped_h16_workspace_bytes(code, m, kdim, ncols))
    assert ws_bytes == env.ops.cbsp_grouped_h16_plan(tdt, m, kdim, ncols, c["k"], c["group_rows"], 256)["workspace"] and ws_bytes % 4 == 0
    wbuf = torch.full((frame + ws_bytes // 4 + frame,), sentinel, dtype=torch.float32, device="cuda")
    results = []
    for _ in range(2):
        y = ybuf[frame: frame + m * ncols]
        nat.check(L.nnc_cbsp_grouped_h16(x_t.data_ptr(), code, m, kdim, codes.buf.data_ptr(), codes.buf.numel(), ncols, codes.zero_symbols.data_ptr(),
                                         codes.nnz, cen_t.data_ptr(), c["k"], c["group_rows"], None if bias_t is None else bias_t.data_ptr(), 0,
                                         y.data_ptr(), code if y_half else 0, wbuf[frame:].data_ptr() if ws_bytes else None, ws_bytes,
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        results.append(y.clone().view(m, ncols))
        for buf, n in ((ybuf, m * ncols), (wbuf, ws_bytes // 4)):
            assert (buf[:frame] == sentinel).all() and (buf[frame + n:] == sentinel).all()
    assert _same(results[0], results[1])
    assert _same(results[0], _op(env, x_t, d, cen_t, bias_t, False, None if y_half else torch.float32))
    assert torch.isfinite(results[0].float()).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_16_rows_and_17_rows_agree_on_exact_data(env, dtype):
    """The stream path at m = 16 and the MFMA path at m = 17 compute the same function where every sum is exact."""
    c = ref._case(17, 300, 129, 16, group_rows=64)
    lab, zs, x, cen, bias = ref.exact_data(c, 77, 0)
    cen_r = grouped_ref.round_centres(cen, dtype)
    assert 4.0 * ref._magnitude(x, lab, cen_r, zs, 64, bias).max() < 2.0 ** 24
    codes = env.ops.pack_grouped_sparse_codes(_dev_labels(lab), 300, 129, 16, 64, zero_symbols=torch.from_numpy(zs).cuda())
    d = dict(codes=codes)
    cen_t, bias_t = _dev(cen), _dev(bias)
    y17 = _op(env, _half(x, dtype), d, cen_t, bias_t, out_dtype=torch.float32)
    y16 = _op(env, _half(x[:16], dtype), d, cen_t, bias_t, out_dtype=torch.float32)
    assert np.array_equal(y17.cpu().numpy().astype(np.float64), ref.formula64(x, lab, cen_r, zs, 64, bias))
    assert torch.equal(y17[:16], y16)


# ------------------------------------------------------------------ 7. label and centre edges
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [4, 40])
def test_no_stored_symbol_at_all_and_an_fp16_centre_of_1e5(env, m, dtype):
    """nnz = 0: every label is its group's z, so W_h is rn(c_{z_g}) throughout (group 1: z past K, 0).  Then a centre of 1e5 stored
    where labels point: Inf in fp16, 99840 in bf16, through both paths as through their references."""
    ops, tdt = env.ops, h16_ref.torch_dtype(dtype)
    rng = np.random.RandomState(m)
    kdim, ncols, k, rows = 96, 70, 8, 32
    zs = np.array([2, 200, 5], dtype=np.uint8)
    lab = np.repeat(zs.astype(np.int64), rows)[:, None].repeat(ncols, axis=1)
    cen = rng.randint(-8, 9, size=(3, k)).astype(np.float32)
    x = rng.randint(-3, 4, size=(m, kdim)).astype(np.float32)
    zs_t = torch.from_numpy(zs).cuda()
    empty = ops.pack_grouped_sparse_codes(_dev_labels(lab), kdim, ncols, k, rows, zero_symbols=zs_t)
    assert empty.nnz == 0
    y = _op(env, _half(x, dtype), dict(codes=empty), _dev(cen), out_dtype=torch.float32).cpu().numpy()
    assert np.array_equal(y.astype(np.float64), x.astype(np.float64) @ grouped_ref.weights(cen, lab, kdim, ncols, rows).astype(np.float64))
    lab2 = lab.copy()
    lab2[::3, ::2] = 7
    big = cen.copy()
    big[:, 7] = 1e5
    codes = ops.pack_grouped_sparse_codes(_dev_labels(lab2), kdim, ncols, k, rows, zero_symbols=zs_t)
    x_t, big_t = _half(np.abs(x) + 1, dtype), _dev(big)
    y = _op(env, x_t, dict(codes=codes), big_t, out_dtype=torch.float32)
    with torch.no_grad():
        if m > 16:
            want = ops.grouped_codebook_matmul(x_t, codes.to_dense(), big_t, kdim, ncols, rows, out_dtype=torch.float32)
        else:
            want = ops.grouped_sparse_codebook_matmul(x_t.float(), codes, big_t.to(tdt).float())
    assert _same(y, want)
    assert bool(torch.isinf(y[:, ::2]).all()) == (dtype == "fp16") and torch.isfinite(y[:, 1::2]).all()


# ------------------------------------------------------------------ the op's rules
def test_the_op_keeps_its_refusals_and_a_float32_x_takes_the_same_call(env, case_data):
    ops = env.ops
    c, d = CASES[0], case_data[0]
    x_t, cen_t = _dev(d["x"]), _dev(d["cen"])
    bias_t = None if d["bias"] is None else _dev(d["bias"])
    xh = x_t.to(torch.bfloat16)
    with torch.no_grad():
        plain = ops.grouped_sparse_codebook_matmul(x_t, d["codes"], cen_t, bias=bias_t)
        assert _same(plain, ops.grouped_sparse_codebook_matmul(x_t, d["codes"], cen_t, bias=bias_t, half_inputs=True))
        assert _same(plain, ops.grouped_sparse_codebook_matmul(x_t, d["codes"], cen_t, bias=bias_t, out_dtype=torch.float32, half_inputs=True))
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="float32 activations.*half_inputs=True"):
            ops.grouped_sparse_codebook_matmul(x_t.to(dt), d["codes"], cen_t)
        with pytest.raises(TypeError, match="centers"):
            ops.grouped_sparse_codebook_matmul(xh, d["codes"], cen_t.to(dt), half_inputs=True)
        with pytest.raises(TypeError, match="bias"):
            ops.grouped_sparse_codebook_matmul(xh, d["codes"], cen_t, bias=torch.zeros(c["ncols"], dtype=dt, device="cuda"), half_inputs=True)
    with pytest.raises(TypeError, match="float32"):
        ops.grouped_sparse_codebook_matmul(x_t.double(), d["codes"], cen_t, half_inputs=True)
    for x_bad, od in ((xh, torch.float16), (xh, torch.bfloat16), (xh, torch.float64), (x_t, torch.bfloat16), (x_t.to(torch.float16), torch.bfloat16)):
        with pytest.raises(TypeError, match="out_dtype"):
            ops.grouped_sparse_codebook_matmul(x_bad, d["codes"], cen_t, out_dtype=od, half_inputs=True)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.grouped_sparse_codebook_matmul(xh.clone().requires_grad_(True), d["codes"], cen_t, half_inputs=True)
    with pytest.raises(ValueError, match="centers must have shape"):
        ops.grouped_sparse_codebook_matmul(xh, d["codes"], cen_t[:1], half_inputs=True)
    with torch.no_grad():
        y3 = ops.grouped_sparse_codebook_matmul(xh.view(1, c["m"], c["kdim"]), d["codes"], cen_t, half_inputs=True)
        assert y3.shape == (1, c["m"], c["ncols"]) and y3.dtype == torch.bfloat16
        assert ops.grouped_sparse_codebook_matmul(xh[:0], d["codes"], cen_t, half_inputs=True).shape == (0, c["ncols"])
    # kdim = 0 writes the bias, rounded once to the output's dtype, at both row counts
    empty = ops.pack_grouped_sparse_codes(torch.zeros(0, dtype=torch.uint8, device="cuda"), 0, 5, 4, 32)
    bias = torch.tensor([-2.0, -1.0, 0.0, 1.0009765625, 3.0], device="cuda")
    for m in (3, 20):
        for dt in (torch.bfloat16, torch.float16):
            with torch.no_grad():
                y0 = ops.grouped_sparse_codebook_matmul(torch.zeros(m, 0, dtype=dt, device="cuda"), empty, torch.zeros(1, 4, device="cuda"), bias=bias,
                                                        relu=True, half_inputs=True)
            assert _same(y0, torch.relu(bias).to(dt).expand(m, 5).contiguous())


# ------------------------------------------------------------------ 8. the layer and the network functions
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


def _grouped_layer(compressed, rng, kdim, ncols, k, rows, density, activation):
    c = dict(kdim=kdim, ncols=ncols, k=k, group_rows=rows)
    zs = (1 + 2 * np.arange(ref.groups_of(c))) % k
    lab = np.concatenate([sparse_ref.labels_at_density(rng, min(kdim, (g + 1) * rows) - g * rows, ncols, k, density, int(z))
                          for g, z in enumerate(zs)], axis=0)
    cen = (rng.standard_normal((len(zs), k)) * 0.2).astype(np.float32)
    bias = rng.standard_normal(ncols).astype(np.float32)
    return compressed.GroupedCompressedDense.from_codes(kdim, ncols, rows, _dev_labels(lab, 1), _dev(cen), _dev(bias), activation)


@pytest.mark.parametrize("m", [5, 40])
def test_the_layer_and_the_network_functions_run_half_inputs_end_to_end(env, m):
    from neural_network_compression_amd import compressed

    ops = env.ops
    rng = np.random.RandomState(21 + m)
    l1 = _grouped_layer(compressed, rng, 96, 64, 16, 32, 0.1, torch.relu)
    l2 = _grouped_layer(compressed, rng, 64, 10, 16, 32, 0.1, None)
    net = _Net(fc1=l1, fc2=l2)
    x32 = _dev(rng.standard_normal((m, 96)))
    with torch.no_grad():
        for dt in (torch.bfloat16, torch.float16):
            xh = x32.to(dt)
            layer = compressed.GroupedSparseCompressedDense.from_grouped(l1, half_inputs=True)
            assert layer.half_inputs is True
            y = layer(xh)
            assert y.dtype == dt and _same(y, ops.grouped_sparse_codebook_matmul(xh, layer.codes, layer.centers, bias=layer.bias, relu=True, half_inputs=True))
            plain = compressed.GroupedSparseCompressedDense.from_grouped(l1)
            assert plain.half_inputs is False and _same(layer(x32), plain(x32))   # a float32 input: the plain layer bit for bit
            with pytest.raises(TypeError, match="float32 activations"):
                plain(xh)

            full = compressed.sparsify_grouped_layers(net, half_inputs=True)
            assert type(full.fc1) is type(full.fc2) is compressed.GroupedSparseCompressedDense and full.fc1.half_inputs and full.fc2.half_inputs
            auto = compressed.sparsify_grouped_layers(net, sparse="auto", half_inputs=True)
            assert type(auto.fc1) is compressed.GroupedSparseCompressedDense and type(auto.fc2) is compressed.GroupedCompressedDense
            small = compressed.smallest_grouped_layers(net, half_inputs=True)
            picked = compressed.smallest_grouped_layers(net)
            assert [type(v) for v in small.get_config().values()] == [type(v) for v in picked.get_config().values()]   # the same forms are picked
            assert type(small.fc1) is compressed.GroupedSparseCompressedDense and small.fc1.half_inputs
            for made in (full, auto, small):
                out = made(xh)
                assert out.dtype == dt and out.shape == (m, 10) and torch.isfinite(out).all()
                h = made.fc1(xh)
                assert _same(out, made.fc2(h)) and _same(made(xh), out)
                if m > 16:   # every layer is the byte form's function bit for bit from 17 rows on
                    assert _same(out, net(xh))
            for default in (compressed.sparsify_grouped_layers(net), picked):
                assert default.fc1.half_inputs is False
                with pytest.raises(TypeError, match="float32 activations"):
                    default(xh)
            assert _same(full(x32), compressed.sparsify_grouped_layers(net)(x32))
    with pytest.raises(RuntimeError, match="inference only"):
        layer(x32.to(torch.bfloat16).requires_grad_(True))
    clone = compressed.GroupedSparseCompressedDense.from_grouped(l1, half_inputs=True)
    clone.load_state_dict(layer.state_dict())
    with torch.no_grad():
        assert _same(clone(xh), layer(xh))
