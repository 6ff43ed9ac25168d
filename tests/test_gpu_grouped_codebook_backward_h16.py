"""The backward pass of the group-wise codebook matmul on bf16 / fp16 activations (nnc_cbmm_grouped_dx_h16 /
nnc_cbmm_grouped_dc_h16, csrc/nnc_cbgrad_grouped_h16.hip), ops.grouped_codebook_linear(half_inputs=True), the
trainable layer built with half_inputs=True and Trainer.fine_tune_grouped(activation_dtype=...) (run with -m gpu).

Every reference is an entry point that existed before, so no tolerance appears:
1. every group's columns of dx equal the half ops.codebook_matmul_dx with that group's one table;
2. dc equals the half ops.codebook_centroid_grad on the 16-bit labels q * K + label with G * K bins;
4. with one group all calls equal the ungrouped half calls;
5. at m <= 16 with float32 output they equal the float32 grouped entry points on the widened inputs;
all bit for bit (NaN payloads included: the comparisons are on the bits).  Exact data also gives the float64 formulas."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import grouped_h16_grad_ref as ref  # noqa: E402
from tests.helpers.h16_ref import DT_CODE, DTYPES, torch_dtype  # noqa: E402

IDS = [ref.case_id(c) for c in ref.CASES]
NAN16 = {"bf16": 0x7FC1, "fp16": 0x7E01}


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, ops

    _native.load()
    _, cus = ops.device_info()
    return ops, cus


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _dev_labels(lab, off, dtype=np.uint8):
    """The indices ``off`` elements into a buffer that ends with them."""
    host = np.ascontiguousarray(lab.astype(dtype)).ravel()
    if dtype == np.uint16:
        host = host.view(np.int16)
    buf = torch.zeros(off + host.size, dtype=torch.uint8 if dtype == np.uint8 else torch.int16, device="cuda")
    buf[off:] = torch.from_numpy(host).cuda()
    return buf[off:]


def _half(a, dt, view):
    """``a`` as a contiguous dt tensor inside a buffer of NaN bit patterns: at element 1 of it (2 bytes off every alignment) for a
    view, at its head else; NaNs lie directly behind the last element either way."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(torch_dtype(dt))
    off = 1 if view else 0
    buf = torch.full((off + t.numel() + 16,), NAN16[dt], dtype=torch.int16, device="cuda").view(torch_dtype(dt))
    buf[off: off + t.numel()] = t.reshape(-1)
    return buf[off: off + t.numel()].view(t.shape)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dims(c):
    return c["m"], c["kdim"], c["ncols"], c["k"], c["group_rows"]


def _run(ops, c, dt, x, g, cen, lab):
    m, kdim, ncols, k, gr = _dims(c)
    labels = _dev_labels(lab, c["off"])
    xt, gt, ct = _half(x, dt, c["view"]), _half(g, dt, c["view"]), _cuda(cen)
    return dict(lab=lab, labels=labels, xt=xt, gt=gt, ct=ct,
                dx=ops.grouped_codebook_matmul_dx(gt, labels, ct, kdim, ncols, gr),
                dx32=ops.grouped_codebook_matmul_dx(gt, labels, ct, kdim, ncols, gr, out_dtype=torch.float32),
                dc=ops.grouped_codebook_centroid_grad(xt, gt, labels, k, kdim, ncols, gr),
                dc32=ops.grouped_codebook_centroid_grad(xt, gt, labels, k, kdim, ncols, gr, dtype=torch.float32))


@pytest.fixture(scope="module")
def float_runs(env):
    """Every case once per dtype on float data, with and without indices beyond K (left unchanged)."""
    ops, _ = env
    runs = {}

    def run(case, dt, oob):
        key = (ref.case_id(case), dt, oob)
        if key not in runs:
            m, kdim, ncols, k, gr = _dims(case)
            x, g, cen = ref.float_data(case, seed=m)
            runs[key] = _run(ops, case, dt, x, g, cen, ref.labels_of(case, seed=kdim + ncols, oob=oob))
        return runs[key]

    return run


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ref.CASES + ref.EMPTY_CASES, ids=IDS + [ref.case_id(c) for c in ref.EMPTY_CASES])
def test_exact_data_matches_float64_bit_for_bit(env, case, dt):
    ops, _ = env
    m, kdim, ncols, k, gr = _dims(case)
    lab = ref.labels_of(case, seed=3 * m + kdim, oob=k < 254)
    x, g, cen = ref.exact_data(case, seed=m + ncols)
    r = _run(ops, case, dt, x, g, cen, lab)
    want_dx = torch.from_numpy(ref.dx64(case, g, lab, cen).astype(np.float32)).cuda()
    want_dc = ref.dc64(case, x, g, lab)
    assert r["dx32"].dtype == torch.float32 and r["dx"].dtype == torch_dtype(dt) and r["dx"].shape == (m, kdim)
    assert torch.equal(r["dx32"], want_dx)
    assert torch.equal(r["dx"], want_dx.to(torch_dtype(dt)))
    assert r["dc"].shape == (ref.groups_of(case), k)
    assert np.array_equal(r["dc"].cpu().numpy(), want_dc)
    assert np.array_equal(r["dc32"].cpu().numpy(), want_dc.astype(np.float32))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("oob", [False, True], ids=["inK", "beyondK"])
@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_dx_equals_the_ungrouped_half_kernel_group_by_group(env, float_runs, case, oob, dt):
    """identity 1, float32 and half output"""
    ops, _ = env
    m, kdim, ncols, k, gr = _dims(case)
    r = float_runs(case, dt, oob)
    for q in range(ref.groups_of(case)):
        rows = ref.group_rows_of(case, q)
        table = r["ct"][q].contiguous()
        one = ops.codebook_matmul_dx(r["gt"], r["labels"], table, kdim, ncols)
        one32 = ops.codebook_matmul_dx(r["gt"], r["labels"], table, kdim, ncols, out_dtype=torch.float32)
        assert _same(r["dx"][:, rows], one[:, rows]), q
        assert _same(r["dx32"][:, rows], one32[:, rows]), q


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_dc_equals_the_ungrouped_half_kernel_on_16_bit_labels(env, float_runs, case, dt):
    """identity 2, float64 and float32 output"""
    ops, _ = env
    m, kdim, ncols, k, gr = _dims(case)
    r = float_runs(case, dt, False)
    gk = ref.groups_of(case) * k
    assert gk <= 1040
    lab16 = _dev_labels(ref.labels16(case, r["lab"]), 0, dtype=np.uint16)
    for out, got in ((torch.float64, r["dc"]), (torch.float32, r["dc32"])):
        want = ops.codebook_centroid_grad(r["xt"], r["gt"], lab16, gk, kdim, ncols, dtype=out)
        assert _same(got.reshape(-1), want), out
    assert float(r["dc"].abs().sum()) > 0


WIDE_CASES = [c for c in ref.CASES if c["k"] <= 253 and ref.groups_of(c) * (c["k"] + 3) <= 1040]   # room for three more bins per group


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", WIDE_CASES, ids=[ref.case_id(c) for c in WIDE_CASES])
def test_labels_beyond_k_fall_into_no_bin(env, float_runs, case, dt):
    """dc with labels >= K equals dc on the same data with those weights' products removed: the float64 formula on exact data
    covers the values; here the identity with the ungrouped kernel at K + 3 bins per group, of which the first K are compared."""
    ops, _ = env
    m, kdim, ncols, k, gr = _dims(case)
    r = float_runs(case, dt, True)
    wide = dict(case, k=k + 3)
    lab16 = _dev_labels(ref.labels16(wide, r["lab"]), 0, dtype=np.uint16)
    want = ops.codebook_centroid_grad(r["xt"], r["gt"], lab16, ref.groups_of(case) * (k + 3), kdim, ncols).reshape(-1, k + 3)
    # the wide call has more bins but the same terms, tiles and splits: the same S, so the same bits in the bins both have
    assert _same(r["dc"], want[:, :k].contiguous())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ref.ONE_GROUP_CASES, ids=[ref.case_id(c) for c in ref.ONE_GROUP_CASES])
def test_one_group_is_the_ungrouped_half_call(env, float_runs, case, dt):
    """identity 4"""
    ops, _ = env
    m, kdim, ncols, k, gr = _dims(case)
    r = float_runs(case, dt, True)
    c1 = r["ct"][0].contiguous()
    assert _same(r["dx"], ops.codebook_matmul_dx(r["gt"], r["labels"], c1, kdim, ncols))
    assert _same(r["dx32"], ops.codebook_matmul_dx(r["gt"], r["labels"], c1, kdim, ncols, out_dtype=torch.float32))
    assert _same(r["dc"].reshape(-1), ops.codebook_centroid_grad(r["xt"], r["gt"], r["labels"], k, kdim, ncols))
    assert _same(r["dc32"].reshape(-1), ops.codebook_centroid_grad(r["xt"], r["gt"], r["labels"], k, kdim, ncols, dtype=torch.float32))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("oob", [False, True], ids=["inK", "beyondK"])
@pytest.mark.parametrize("case", [c for c in ref.CASES if c["m"] <= 16], ids=[ref.case_id(c) for c in ref.CASES if c["m"] <= 16])
def test_the_stream_path_is_the_float32_grouped_kernel_on_widened_inputs(env, float_runs, case, oob, dt):
    """identity 5"""
    ops, _ = env
    m, kdim, ncols, k, gr = _dims(case)
    r = float_runs(case, dt, oob)
    xf, gf, cf = r["xt"].float(), r["gt"].float(), r["ct"].to(torch_dtype(dt)).float()
    assert _same(r["dx32"], ops.grouped_codebook_matmul_dx(gf, r["labels"], cf, kdim, ncols, gr))
    assert _same(r["dc"], ops.grouped_codebook_centroid_grad(xf, gf, r["labels"], k, kdim, ncols, gr))
    assert _same(r["dc32"], ops.grouped_codebook_centroid_grad(xf, gf, r["labels"], k, kdim, ncols, gr, dtype=torch.float32))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", [ref.STREAM_CASES[2], ref.MFMA_CASES[0], ref.MFMA_CASES[2]], ids=ref.case_id)
def test_a_second_call_gives_the_same_bits(env, float_runs, case, dt):
    ops, _ = env
    m, kdim, ncols, k, gr = _dims(case)
    r = float_runs(case, dt, True)
    assert _same(r["dx"], ops.grouped_codebook_matmul_dx(r["gt"], r["labels"], r["ct"], kdim, ncols, gr))
    assert _same(r["dc"], ops.grouped_codebook_centroid_grad(r["xt"], r["gt"], r["labels"], k, kdim, ncols, gr))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("gr", [32, 96, 128])
def test_m16_and_m17_agree_on_exact_data(env, dt, gr):
    """The stream and the MFMA kernels sum in different orders; on exact data both are exact, so rows 0..15 agree bit for bit."""
    ops, _ = env
    c17 = dict(m=17, kdim=300, ncols=130, k=16, group_rows=gr, off=1, view=False)
    lab = ref.labels_of(c17, seed=gr, oob=True)
    x, g, cen = ref.exact_data(c17, seed=gr)
    r17 = _run(ops, c17, dt, x, g, cen, lab)
    r16 = _run(ops, dict(c17, m=16), dt, x[:16], g[:16], cen, lab)
    assert torch.equal(r17["dx"][:16], r16["dx"]) and torch.equal(r17["dx32"][:16], r16["dx32"])
    x0, g0 = x.copy(), g.copy()
    x0[16], g0[16] = 0, 0                       # a seventeenth row of zeros adds nothing to dc
    assert torch.equal(_run(ops, c17, dt, x0, g0, cen, lab)["dc"], r16["dc"])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("m", [5, 17, 130])
@pytest.mark.parametrize("gr", [32, 96, 128, 320])
def test_lane_maps_show_a_wrong_table_at_once(env, dt, m, gr):
    """centers[q] = q + 1 everywhere and g = 1: dx[r, i] = ncols * (i // group_rows + 1).  x = 1 and g = 1: dc[q, k] = m * (the count of
    label k in group q)."""
    ops, _ = env
    kdim, ncols, k = 300, 130, 16
    c = dict(m=m, kdim=kdim, ncols=ncols, k=k, group_rows=gr, off=1, view=False)
    G = ref.groups_of(c)
    lab = ref.labels_of(c, seed=m + gr)
    cen = np.repeat(np.arange(1, G + 1, dtype=np.float32)[:, None], k, axis=1)
    r = _run(ops, c, dt, np.ones((m, kdim), np.float32), np.ones((m, ncols), np.float32), cen, lab)
    want_dx = np.broadcast_to(ncols * (np.arange(kdim) // gr + 1.0), (m, kdim)).astype(np.float32)
    assert np.array_equal(r["dx32"].cpu().numpy(), want_dx)
    counts = np.stack([np.bincount(lab[ref.group_rows_of(c, q)].ravel(), minlength=k) for q in range(G)])
    assert np.array_equal(r["dc"].cpu().numpy(), (m * counts).astype(np.float64))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", [ref.STREAM_CASES[2], ref.STREAM_CASES[3], ref.MFMA_CASES[0], ref.MFMA_CASES[2]], ids=ref.case_id)
def test_sentinel_frames_around_dx_dc_and_the_workspace(env, case, dt):
    """The native calls on buffers framed by sentinels: nothing outside dx, dc and the workspace the query asked for is written, and
    the results are those of the ops calls."""
    ops, _ = env
    from neural_network_compression_amd import _native as nat

    L = nat.load()
    m, kdim, ncols, k, gr = _dims(case)
    G = ref.groups_of(case)
    x, g, cen = ref.float_data(case, seed=m)
    lab = ref.labels_of(case, seed=kdim + ncols, oob=True)
    r = _run(ops, case, dt, x, g, cen, lab)
    code, s = DT_CODE[dt], torch.cuda.current_stream().cuda_stream
    PAD = 64

    def framed(nbytes):
        buf = torch.full((PAD + nbytes + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        return buf, buf[PAD: PAD + nbytes]

    def intact(buf, nbytes):
        return bool((buf[:PAD] == 0xA5).all()) and bool((buf[PAD + nbytes:] == 0xA5).all())

    for out_code, want in ((code, r["dx"]), (0, r["dx32"])):
        nb = m * kdim * (4 if out_code == 0 else 2)
        ws_bytes = int(L.nnc_cbmm_grouped_dx_h16_workspace_bytes(m, kdim, ncols))
        dbuf, dx = framed(nb)
        wbuf, ws = framed(ws_bytes)
        nat.check(L.nnc_cbmm_grouped_dx_h16(r["gt"].data_ptr(), code, m, kdim, r["labels"].data_ptr(), ncols, r["ct"].data_ptr(), k, gr, dx.data_ptr(),
                                            out_code, ws.data_ptr() if ws_bytes else None, ws_bytes, s))
        torch.cuda.synchronize()
        assert intact(dbuf, nb) and intact(wbuf, ws_bytes)
        assert _same(dx.view(want.dtype).view(m, kdim), want)
    for f64, want in ((1, r["dc"]), (0, r["dc32"])):
        nb = G * k * (8 if f64 else 4)
        ws_bytes = int(L.nnc_cbmm_grouped_dc_h16_workspace_bytes(m, kdim, ncols, k, gr))
        assert ws_bytes == 64 + 8 * G * k
        dbuf, dc = framed(nb)
        wbuf, ws = framed(ws_bytes)
        nat.check(L.nnc_cbmm_grouped_dc_h16(r["xt"].data_ptr(), r["gt"].data_ptr(), code, m, kdim, r["labels"].data_ptr(), ncols, k, gr, dc.data_ptr(), f64,
                                            ws.data_ptr(), ws_bytes, s))
        torch.cuda.synchronize()
        assert intact(dbuf, nb) and intact(wbuf, ws_bytes)
        assert _same(dc.view(want.dtype).view(G, k), want)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("m", [16, 17])
def test_inf_and_nan_on_both_sides_of_m16(env, dt, m):
    """A non-finite g reaches exactly the dx rows the ungrouped kernel gives it (bit for bit, per group); a non-finite x or g makes
    every dc NaN; a zero maximum makes dc 0."""
    ops, _ = env
    c = dict(m=m, kdim=200, ncols=130, k=16, group_rows=96, off=1, view=True)
    kdim, ncols, k, gr = c["kdim"], c["ncols"], c["k"], c["group_rows"]
    lab = ref.labels_of(c, seed=5, oob=True)
    x, g, cen = ref.float_data(c, seed=m)
    gbad = g.copy()
    gbad[0, 3], gbad[m - 1, 129], gbad[1, 64] = np.inf, -np.inf, np.nan
    r = _run(ops, c, dt, x, gbad, cen, lab)
    for q in range(ref.groups_of(c)):
        rows = ref.group_rows_of(c, q)
        one = ops.codebook_matmul_dx(r["gt"], r["labels"], r["ct"][q].contiguous(), kdim, ncols)
        assert _same(r["dx"][:, rows], one[:, rows])
    assert bool(torch.isfinite(r["dx32"][2:m - 1]).all()) and not bool(torch.isfinite(r["dx32"][0]).all())
    assert bool(torch.isnan(r["dc"]).all()) and bool(torch.isnan(r["dc32"]).all())
    xbad = x.copy()
    xbad[m - 1, 199] = np.nan
    assert bool(torch.isnan(_run(ops, c, dt, xbad, g, cen, lab)["dc"]).all())
    z = _run(ops, c, dt, x, np.zeros_like(g), cen, lab)
    assert not bool(z["dc"].any()) and not bool(z["dx32"].any())


@pytest.mark.parametrize("m", [16, 17, 130])
def test_bf16_dc_at_tiny_magnitudes_and_around_p127(env, m):
    """bf16 has float32's exponent range: x and g near 2^-80 (products near 2^-160) are scaled into range, and the all-NaN rule sets
    in exactly where 2^P > m * max|x| * max|g| passes P = 127 -- the ungrouped kernel's behaviour, bit for bit."""
    ops, _ = env
    c = dict(m=m, kdim=200, ncols=50, k=16, group_rows=96, off=0, view=False)
    kdim, ncols, k, gr = c["kdim"], c["ncols"], c["k"], c["group_rows"]
    lab = ref.labels_of(c, seed=9)
    x, g, cen = ref.exact_data(c, seed=m)
    lab16 = _dev_labels(ref.labels16(c, lab), 0, dtype=np.uint16)
    gk = ref.groups_of(c) * k
    tiny = _run(ops, c, "bf16", x * np.float32(2.0 ** -80), g * np.float32(2.0 ** -80), cen, lab)
    assert np.array_equal(tiny["dc"].cpu().numpy(), ref.dc64(c, x, g, lab) * 2.0 ** -160) and float(tiny["dc"].abs().sum()) > 0
    e = 127 - int(np.ceil(np.log2(m * 9.0)))          # |x|, |g| <= 3: m * 9 * 2^e stays below 2^127, one more doubling passes it
    for shift, nan in ((e - 2, False), (e + 3, True)):
        big = _run(ops, c, "bf16", x * np.float32(2.0 ** 60), g * np.float32(2.0 ** (shift - 60)), cen, lab)
        want = ops.codebook_centroid_grad(big["xt"], big["gt"], lab16, gk, kdim, ncols)
        assert _same(big["dc"].reshape(-1), want)
        assert bool(torch.isnan(big["dc"]).all()) == nan


@pytest.mark.parametrize("m", [16, 17])
def test_fp16_at_65504_beside_subnormals(env, m):
    ops, _ = env
    c = dict(m=m, kdim=200, ncols=50, k=16, group_rows=96, off=0, view=False)
    kdim, ncols, k, gr = c["kdim"], c["ncols"], c["k"], c["group_rows"]
    lab = ref.labels_of(c, seed=11)
    rng = np.random.RandomState(m)
    x = rng.choice(np.array([65504.0, -65504.0, 2.0 ** -24, -2.0 ** -22, 1.0, 0.0], dtype=np.float32), size=(m, kdim))
    g = rng.choice(np.array([65504.0, 2.0 ** -24, -2.0 ** -20, 0.5, 0.0], dtype=np.float32), size=(m, ncols))
    cen = rng.choice(np.array([65504.0, -2.0 ** -24, 2.0 ** -14, 1.5], dtype=np.float32), size=(ref.groups_of(c), k))
    r = _run(ops, c, "fp16", x, g, cen, lab)
    lab16 = _dev_labels(ref.labels16(c, lab), 0, dtype=np.uint16)
    assert _same(r["dc"].reshape(-1), ops.codebook_centroid_grad(r["xt"], r["gt"], lab16, ref.groups_of(c) * k, kdim, ncols))
    assert bool(torch.isfinite(r["dc"]).all()) and float(r["dc"].abs().max()) > 0
    for q in range(ref.groups_of(c)):
        rows = ref.group_rows_of(c, q)
        assert _same(r["dx32"][:, rows], ops.codebook_matmul_dx(r["gt"], r["labels"], r["ct"][q].contiguous(), kdim, ncols, out_dtype=torch.float32)[:, rows])


# ------------------------------------------------------------------ the 2- / 4-bit packed form
PIDS = [ref.packed_case_id(c) for c in ref.PACKED_CASES]


@pytest.fixture(scope="module")
def packed_runs(env):
    """Every packed case once per dtype on float data: the byte grouped half results on the unpacked labels and the packed ones."""
    ops, _ = env
    runs = {}

    def run(case, dt):
        key = (ref.packed_case_id(case), dt)
        if key not in runs:
            m, kdim, ncols, k, gr = _dims(case)
            x, g, cen = ref.float_data(case, seed=m)
            lab = ref.packed_labels_of(case, seed=kdim + ncols)
            r = _run(ops, case, dt, x, g, cen, lab)
            codes = ops.pack_codes(r["labels"], kdim, ncols, k, case["bits"])
            r.update(codes=codes,
                     pdx=ops.grouped_packed_codebook_matmul_dx(r["gt"], codes, r["ct"], gr),
                     pdx32=ops.grouped_packed_codebook_matmul_dx(r["gt"], codes, r["ct"], gr, out_dtype=torch.float32),
                     pdc=ops.grouped_packed_codebook_centroid_grad(r["xt"], r["gt"], codes, gr),
                     pdc32=ops.grouped_packed_codebook_centroid_grad(r["xt"], r["gt"], codes, gr, dtype=torch.float32))
            runs[key] = r
        return runs[key]

    return run


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ref.PACKED_CASES, ids=PIDS)
def test_packed_equals_the_byte_grouped_half_calls_on_the_unpacked_labels(env, packed_runs, case, dt):
    """identity 3"""
    r = packed_runs(case, dt)
    assert r["codes"].bits == case["bits"] and float(r["dc"].abs().sum()) > 0
    assert _same(r["pdx"], r["dx"]) and _same(r["pdx32"], r["dx32"])
    assert _same(r["pdc"], r["dc"]) and _same(r["pdc32"], r["dc32"])


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", [c for c in ref.PACKED_CASES if c["group_rows"] >= c["kdim"]],
                         ids=[ref.packed_case_id(c) for c in ref.PACKED_CASES if c["group_rows"] >= c["kdim"]])
def test_packed_one_group_is_the_ungrouped_packed_half_call(env, packed_runs, case, dt):
    """identity 4"""
    ops, _ = env
    r = packed_runs(case, dt)
    c1 = r["ct"][0].contiguous()
    assert _same(r["pdx"], ops.packed_codebook_matmul_dx(r["gt"], r["codes"], c1))
    assert _same(r["pdx32"], ops.packed_codebook_matmul_dx(r["gt"], r["codes"], c1, out_dtype=torch.float32))
    assert _same(r["pdc"].reshape(-1), ops.packed_codebook_centroid_grad(r["xt"], r["gt"], r["codes"]))
    assert _same(r["pdc32"].reshape(-1), ops.packed_codebook_centroid_grad(r["xt"], r["gt"], r["codes"], dtype=torch.float32))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", [c for c in ref.PACKED_CASES if c["m"] <= 16], ids=[ref.packed_case_id(c) for c in ref.PACKED_CASES if c["m"] <= 16])
def test_the_packed_stream_path_is_the_float32_kernel_on_widened_inputs(env, packed_runs, case, dt):
    """identity 5"""
    ops, _ = env
    m, kdim, ncols, k, gr = _dims(case)
    r = packed_runs(case, dt)
    xf, gf, cf = r["xt"].float(), r["gt"].float(), r["ct"].to(torch_dtype(dt)).float()
    assert _same(r["pdx32"], ops.grouped_packed_codebook_matmul_dx(gf, r["codes"], cf, gr))
    assert _same(r["pdc"], ops.grouped_packed_codebook_centroid_grad(xf, gf, r["codes"], gr))
    assert _same(r["pdc32"], ops.grouped_packed_codebook_centroid_grad(xf, gf, r["codes"], gr, dtype=torch.float32))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", ref.PACKED_CASES[:9:2], ids=PIDS[:9:2])
def test_packed_exact_data_and_a_second_call(env, case, dt):
    ops, _ = env
    m, kdim, ncols, k, gr = _dims(case)
    lab = ref.packed_labels_of(case, seed=m)
    x, g, cen = ref.exact_data(case, seed=m + ncols)
    xt, gt, ct = _half(x, dt, case["view"]), _half(g, dt, case["view"]), _cuda(cen)
    codes = ops.pack_codes(_dev_labels(lab, 0), kdim, ncols, k, case["bits"])
    dx = ops.grouped_packed_codebook_matmul_dx(gt, codes, ct, gr, out_dtype=torch.float32)
    dc = ops.grouped_packed_codebook_centroid_grad(xt, gt, codes, gr)
    assert np.array_equal(dx.cpu().numpy(), ref.dx64(case, g, lab, cen).astype(np.float32))
    assert np.array_equal(dc.cpu().numpy(), ref.dc64(case, x, g, lab))
    assert _same(dx, ops.grouped_packed_codebook_matmul_dx(gt, codes, ct, gr, out_dtype=torch.float32))
    assert _same(dc, ops.grouped_packed_codebook_centroid_grad(xt, gt, codes, gr))


@pytest.mark.parametrize("m", [5, 17])
@pytest.mark.parametrize("bits,ncols,k", [(4, 33, 16), (2, 70, 4)])
def test_packed_padding_fields_are_never_looked_up(env, m, bits, ncols, k):
    """fp16, centers[q][0] = 1e5 (Inf in fp16) in one group only, and no real weight of label 0: the padding fields past ncols hold
    label 0, and a lookup there would meet the zero of the g image as Inf * 0.  dx is finite and equals the byte form's."""
    ops, _ = env
    kdim, gr = 200, 96
    c = dict(m=m, kdim=kdim, ncols=ncols, k=k, group_rows=gr, off=0, view=False, bits=bits)
    lab = np.random.RandomState(m + bits).randint(1, k, size=(kdim, ncols))
    x, g, cen = ref.float_data(c, seed=m)
    cen[1, 0] = 1e5
    r = _run(ops, c, "fp16", x, g, cen, lab)
    codes = ops.pack_codes(r["labels"], kdim, ncols, k, bits)
    pdx = ops.grouped_packed_codebook_matmul_dx(r["gt"], codes, r["ct"], gr, out_dtype=torch.float32)
    assert bool(torch.isfinite(pdx).all()) and _same(pdx, r["dx32"])
    pdc = ops.grouped_packed_codebook_centroid_grad(r["xt"], r["gt"], codes, gr)
    assert _same(pdc, r["dc"]) and not bool(pdc[:, 0].any())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("m", [5, 17, 130])
@pytest.mark.parametrize("gr,bits,k", [(32, 4, 16), (96, 2, 3), (128, 4, 5), (320, 2, 4)])
def test_packed_lane_maps_show_a_wrong_table_at_once(env, dt, m, gr, bits, k):
    """as the byte form's: centers[q] = q + 1 and g = 1 give dx[r, i] = ncols * (i // group_rows + 1) wherever every label is below K;
    x = g = 1 give dc[q, j] = m * (the count of label j in group q), labels >= K counted nowhere"""
    ops, _ = env
    kdim, ncols = 300, 130
    c = dict(m=m, kdim=kdim, ncols=ncols, k=k, group_rows=gr, off=0, view=False, bits=bits)
    G = ref.groups_of(c)
    lab = ref.packed_labels_of(c, seed=m + gr)
    cen = np.repeat(np.arange(1, G + 1, dtype=np.float32)[:, None], k, axis=1)
    codes = ops.pack_codes(_dev_labels(lab, 0), kdim, ncols, k, bits)
    ones_x, ones_g, ct = _half(np.ones((m, kdim), np.float32), dt, False), _half(np.ones((m, ncols), np.float32), dt, False), _cuda(cen)
    dx = ops.grouped_packed_codebook_matmul_dx(ones_g, codes, ct, gr, out_dtype=torch.float32)
    dc = ops.grouped_packed_codebook_centroid_grad(ones_x, ones_g, codes, gr)
    want_dx = np.broadcast_to((lab < k).sum(1) * (np.arange(kdim) // gr + 1.0), (m, kdim)).astype(np.float32)
    assert np.array_equal(dx.cpu().numpy(), want_dx)
    counts = np.stack([np.bincount(lab[ref.group_rows_of(c, q)].ravel(), minlength=1 << bits)[:k] for q in range(G)])
    assert np.array_equal(dc.cpu().numpy(), (m * counts).astype(np.float64))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("gr,bits,k", [(32, 4, 16), (96, 2, 3)])
def test_packed_m16_and_m17_agree_on_exact_data(env, dt, gr, bits, k):
    ops, _ = env
    c17 = dict(m=17, kdim=300, ncols=130, k=k, group_rows=gr, off=0, view=False, bits=bits)
    lab = ref.packed_labels_of(c17, seed=gr)
    x, g, cen = ref.exact_data(c17, seed=gr)
    codes = ops.pack_codes(_dev_labels(lab, 0), 300, 130, k, bits)
    ct = _cuda(cen)

    def run(xa, ga):
        xt, gt = _half(xa, dt, False), _half(ga, dt, False)
        return (ops.grouped_packed_codebook_matmul_dx(gt, codes, ct, gr), ops.grouped_packed_codebook_matmul_dx(gt, codes, ct, gr, out_dtype=torch.float32),
                ops.grouped_packed_codebook_centroid_grad(xt, gt, codes, gr))

    dx17, dx17f, _ = run(x, g)
    dx16, dx16f, dc16 = run(x[:16], g[:16])
    assert torch.equal(dx17[:16], dx16) and torch.equal(dx17f[:16], dx16f)
    x0, g0 = x.copy(), g.copy()
    x0[16], g0[16] = 0, 0
    assert torch.equal(run(x0, g0)[2], dc16)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", [ref.PACKED_CASES[2], ref.PACKED_CASES[3], ref.PACKED_CASES[4], ref.PACKED_CASES[8]], ids=ref.packed_case_id)
def test_packed_sentinel_frames_around_dx_dc_and_the_workspace(env, packed_runs, case, dt):
    """nnc_cbpk_grouped_dx_h16 / _dc_h16 on buffers framed by sentinels, the packed rows at the very end of their tensor: nothing outside
    dx, dc and the workspace the queries asked for is written, and the results are those of the ops calls."""
    ops, _ = env
    from neural_network_compression_amd import _native as nat

    L = nat.load()
    m, kdim, ncols, k, gr = _dims(case)
    G, bits = ref.groups_of(case), case["bits"]
    r = packed_runs(case, dt)
    codes = r["codes"]
    code, s = DT_CODE[dt], torch.cuda.current_stream().cuda_stream
    PAD = 64

    def framed(nbytes):
        buf = torch.full((PAD + nbytes + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
        return buf, buf[PAD: PAD + nbytes]

    def intact(buf, nbytes):
        return bool((buf[:PAD] == 0xA5).all()) and bool((buf[PAD + nbytes:] == 0xA5).all())

    for out_code, want in ((code, r["pdx"]), (0, r["pdx32"])):
        nb = m * kdim * (4 if out_code == 0 else 2)
        ws_bytes = int(L.nnc_cbpk_grouped_dx_h16_workspace_bytes(m, kdim, ncols, bits))
        dbuf, dx = framed(nb)
        wbuf, ws = framed(ws_bytes)
        nat.check(L.nnc_cbpk_grouped_dx_h16(r["gt"].data_ptr(), code, m, kdim, codes.packed.data_ptr(), codes.nbytes, bits, ncols, r["ct"].data_ptr(), k, gr,
                                            dx.data_ptr(), out_code, ws.data_ptr() if ws_bytes else None, ws_bytes, s))
        torch.cuda.synchronize()
        assert intact(dbuf, nb) and intact(wbuf, ws_bytes)
        assert _same(dx.view(want.dtype).view(m, kdim), want)
    for f64, want in ((1, r["pdc"]), (0, r["pdc32"])):
        nb = G * k * (8 if f64 else 4)
        ws_bytes = int(L.nnc_cbpk_grouped_dc_h16_workspace_bytes(m, kdim, ncols, bits, k, gr))
        assert ws_bytes == 64 + 8 * G * k
        dbuf, dc = framed(nb)
        wbuf, ws = framed(ws_bytes)
        nat.check(L.nnc_cbpk_grouped_dc_h16(r["xt"].data_ptr(), r["gt"].data_ptr(), code, m, kdim, codes.packed.data_ptr(), codes.nbytes, bits, ncols, k, gr,
                                            dc.data_ptr(), f64, ws.data_ptr(), ws_bytes, s))
        torch.cuda.synchronize()
        assert intact(dbuf, nb) and intact(wbuf, ws_bytes)
        assert _same(dc.view(want.dtype).view(G, k), want)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("m", [16, 17])
def test_packed_inf_and_nan_on_both_sides_of_m16(env, dt, m):
    """non-finite g and x through the packed kernels: dx is the byte grouped half dx bit for bit (NaN payloads included), every dc is
    NaN, and a zero maximum makes dc 0"""
    ops, _ = env
    c = dict(m=m, kdim=200, ncols=130, k=5, group_rows=96, off=0, view=True, bits=4)
    kdim, ncols, k, gr = c["kdim"], c["ncols"], c["k"], c["group_rows"]
    lab = ref.packed_labels_of(c, seed=5)
    x, g, cen = ref.float_data(c, seed=m)
    gbad = g.copy()
    gbad[0, 3], gbad[m - 1, 129], gbad[1, 64] = np.inf, -np.inf, np.nan
    r = _run(ops, c, dt, x, gbad, cen, lab)
    codes = ops.pack_codes(r["labels"], kdim, ncols, k, 4)
    assert _same(ops.grouped_packed_codebook_matmul_dx(r["gt"], codes, r["ct"], gr), r["dx"])
    pdx32 = ops.grouped_packed_codebook_matmul_dx(r["gt"], codes, r["ct"], gr, out_dtype=torch.float32)
    assert _same(pdx32, r["dx32"]) and bool(torch.isfinite(pdx32[2:m - 1]).all()) and not bool(torch.isfinite(pdx32[0]).all())
    assert bool(torch.isnan(ops.grouped_packed_codebook_centroid_grad(r["xt"], r["gt"], codes, gr)).all())
    xbad = x.copy()
    xbad[m - 1, 199] = np.nan
    assert bool(torch.isnan(ops.grouped_packed_codebook_centroid_grad(_half(xbad, dt, True), _half(g, dt, True), codes, gr, dtype=torch.float32)).all())
    assert not bool(ops.grouped_packed_codebook_centroid_grad(_half(x, dt, True), _half(np.zeros_like(g), dt, True), codes, gr).any())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("m", [5, 64])
def test_the_byte_and_the_packed_grouped_trainable_layers_agree(env, dt, m):
    """output, x.grad, centers.grad and the gradient of a quantized bias's centres, with a fused ReLU and without, on exact data (on
    float data the byte and the packed forward differ in the order of their float32 sums; the backward calls agree on any data, above)"""
    ops, _ = env
    from neural_network_compression_amd import compressed

    c, lab, _, _, _, bias = _layer_case(dt, m)
    lab = lab % 16
    x, g, cen = ref.exact_data(c, seed=m)             # exact data: the two forward kernels sum in different orders (sections 17, 18)
    bias = np.round(bias * 40) / 4
    kdim, ncols, gr = c["kdim"], c["ncols"], c["group_rows"]
    labels = _dev_labels(lab, 0)
    bias_codes = (_cuda(bias[:8]), _cuda((np.arange(ncols) % 8).astype(np.uint8)))   # a quantized bias: its centres are parameters
    for act in (None, torch.relu):
        outs = []
        layers = (compressed.TrainableGroupedCompressedDense.from_codes(kdim, ncols, gr, labels, _cuda(cen), None, bias_codes, act, half_inputs=True),
                  compressed.TrainableGroupedPackedCompressedDense.from_codes(kdim, ncols, gr, labels, _cuda(cen), None, bias_codes, act, half_inputs=True))
        assert all("half_inputs" in vars(layer) and not hasattr(type(layer), "half_inputs") for layer in layers)
        for layer in layers:
            xt = _half(x, dt, False).requires_grad_(True)
            gt = _half(g, dt, False)
            y = layer(xt)
            y.backward(gt)
            outs.append((y.detach(), xt.grad, layer.centers.grad, layer.bias_centers.grad))
        assert outs[0][0].dtype == torch_dtype(dt) and outs[0][2].dtype == torch.float32
        assert all(_same(a, b) for a, b in zip(*outs))
    with pytest.raises(TypeError, match="float32 activations"):
        compressed.TrainableGroupedPackedCompressedDense.from_codes(kdim, ncols, gr, labels, _cuda(cen))(_half(x, dt, False))
    with pytest.raises(TypeError, match="float32 activations"):
        ops.grouped_packed_codebook_linear(_half(x, dt, False), layers[1].codes, _cuda(cen), gr)


# ------------------------------------------------------------------ autograd and the layers
def _layer_case(dt, m, relu=False, seed=0):
    c = dict(m=m, kdim=300, ncols=130, k=16, group_rows=32, off=0, view=False)
    lab = ref.labels_of(c, seed=seed + 1, oob=True)
    x, g, cen = ref.float_data(c, seed=seed)
    bias = (np.random.RandomState(seed + 5).standard_normal(c["ncols"]) * 0.1).astype(np.float32)
    return c, lab, x, g, cen, bias


def _form_calls(ops, form, labels, kdim, ncols, k, gr):
    """(linear, matmul, dx, dc) of the byte or the packed grouped form on one index matrix, with one signature."""
    if form == "byte":
        return (lambda x, c, **kw: ops.grouped_codebook_linear(x, labels, c, kdim, ncols, gr, **kw),
                lambda x, c, **kw: ops.grouped_codebook_matmul(x, labels, c, kdim, ncols, gr, **kw),
                lambda g, c: ops.grouped_codebook_matmul_dx(g, labels, c, kdim, ncols, gr),
                lambda x, g: ops.grouped_codebook_centroid_grad(x, g, labels, k, kdim, ncols, gr, dtype=torch.float32))
    codes = ops.pack_codes(labels, kdim, ncols, k, 4)
    return (lambda x, c, **kw: ops.grouped_packed_codebook_linear(x, codes, c, gr, **kw),
            lambda x, c, **kw: ops.grouped_packed_codebook_matmul(x, codes, c, gr, **kw),
            lambda g, c: ops.grouped_packed_codebook_matmul_dx(g, codes, c, gr),
            lambda x, g: ops.grouped_packed_codebook_centroid_grad(x, g, codes, gr, dtype=torch.float32))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("m", [5, 64])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("form", ["byte", "packed"])
def test_grouped_linear_with_half_inputs_makes_no_host_read(env, form, dt, m, relu):
    """forward plus backward of ops.grouped_codebook_linear / ops.grouped_packed_codebook_linear (half_inputs=True) under
    set_sync_debug_mode("error"): y, x.grad, centers.grad and bias.grad are those of the form's ops calls, bit for bit"""
    ops, _ = env
    c, lab, x, g, cen, bias = _layer_case(dt, m)
    kdim, ncols, gr, k = c["kdim"], c["ncols"], c["group_rows"], c["k"]
    labels = _dev_labels(lab % 16 if form == "packed" else lab, 0)
    linear, matmul, dx, dc = _form_calls(ops, form, labels, kdim, ncols, k, gr)
    xt = _half(x, dt, False).requires_grad_(True)
    ct, bt, gt = _cuda(cen).requires_grad_(True), _cuda(bias).requires_grad_(True), _half(g, dt, False)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        y = linear(xt, ct, bias=bt, relu=relu, half_inputs=True)
        y.backward(gt)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    with torch.no_grad():
        want_y = matmul(xt, ct, bias=bt, relu=relu)
        gm = torch.where(want_y > 0, gt, torch.zeros((), dtype=gt.dtype, device="cuda")) if relu else gt
        assert y.dtype == torch_dtype(dt) and _same(y.detach(), want_y)
        assert xt.grad.dtype == torch_dtype(dt) and _same(xt.grad, dx(gm, ct))
        assert ct.grad.dtype == torch.float32 and _same(ct.grad, dc(xt.detach(), gm))
        assert bt.grad.dtype == torch.float32 and _same(bt.grad, gm.sum(0, dtype=torch.float32))


def test_without_the_keyword_nothing_changes(env):
    ops, _ = env
    from neural_network_compression_amd import compressed

    c, lab, x, g, cen, bias = _layer_case("bf16", 5)
    kdim, ncols, gr = c["kdim"], c["ncols"], c["group_rows"]
    labels, ct, bt = _dev_labels(lab, 0), _cuda(cen), _cuda(bias)
    xf = _cuda(x)
    for half in (xf.half(), xf.bfloat16()):
        with pytest.raises(TypeError, match="float32 activations"):
            ops.grouped_codebook_linear(half, labels, ct, kdim, ncols, gr)
        with pytest.raises(TypeError, match="float32 activations"):
            compressed.TrainableGroupedCompressedDense(kdim, ncols, gr, labels, ct, bt)(half)
        with pytest.raises(TypeError):                               # half centres or bias stay an error with the keyword too
            ops.grouped_codebook_linear(half, labels, ct.to(half.dtype), kdim, ncols, gr, half_inputs=True)
        with pytest.raises(TypeError):
            ops.grouped_codebook_linear(half, labels, ct, kdim, ncols, gr, bias=bt.to(half.dtype), half_inputs=True)
        with pytest.raises(TypeError):                               # mixed dtypes
            ops.grouped_codebook_centroid_grad(half, _cuda(g), labels, c["k"], kdim, ncols, gr)
        with pytest.raises(TypeError):
            ops.grouped_codebook_matmul_dx(_cuda(g).to(half.dtype), labels, ct, kdim, ncols, gr, out_dtype=torch.float64)
    with pytest.raises(TypeError):
        ops.grouped_codebook_matmul_dx(_cuda(g), labels, ct, kdim, ncols, gr, out_dtype=torch.bfloat16)
    # float32 through the layer, with and without the keyword: the same bits forward and backward
    lab16 = _dev_labels(lab % 16, 0)
    for cls, idx in ((compressed.TrainableGroupedCompressedDense, labels), (compressed.TrainableGroupedPackedCompressedDense, lab16)):
        outs = []
        for kw in ({}, dict(half_inputs=True)):
            layer = cls.from_codes(kdim, ncols, gr, idx, ct, bt, None, torch.relu, **kw)
            assert ("half_inputs" in vars(layer)) and not hasattr(cls, "half_inputs") and layer.half_inputs == bool(kw)
            xin = xf.clone().requires_grad_(True)
            layer(xin).backward(_cuda(g))
            outs.append((layer(xin).detach(), xin.grad, layer.centers.grad))
        assert all(_same(a, b) for a, b in zip(*outs)), cls
        gm = torch.where(outs[0][0] > 0, _cuda(g), torch.zeros((), device="cuda"))
        want = (ops.grouped_packed_codebook_matmul_dx(gm, layer.codes, ct, gr) if cls is compressed.TrainableGroupedPackedCompressedDense else
                ops.grouped_codebook_matmul_dx(gm, idx, ct, kdim, ncols, gr))
        assert _same(outs[0][1], want), cls
    for half in (xf.half(), xf.bfloat16()):
        with pytest.raises(TypeError, match="float32 activations"):
            compressed.TrainableGroupedPackedCompressedDense.from_codes(kdim, ncols, gr, lab16, ct, bt)(half)


@pytest.mark.parametrize("dt", DTYPES)
def test_two_layer_exact_chain_against_float64_autograd(env, dt):
    ops, _ = env
    from neural_network_compression_amd import compressed

    m, d0, d1, d2, gr, k = 17, 96, 64, 40, 32, 4
    rng = np.random.RandomState(3)
    x = rng.randint(-2, 3, size=(m, d0)).astype(np.float32)
    lab1, lab2 = rng.randint(0, k, size=(d0, d1)), rng.randint(0, k, size=(d1, d2))
    cen1 = rng.randint(-2, 3, size=(d0 // gr, k)).astype(np.float32) / 2
    cen2 = rng.randint(-2, 3, size=(d1 // gr, k)).astype(np.float32) / 2
    gy = rng.randint(-2, 3, size=(m, d2)).astype(np.float32)
    l1 = compressed.TrainableGroupedCompressedDense(d0, d1, gr, _dev_labels(lab1, 0), _cuda(cen1), None, None, torch.relu, half_inputs=True)
    l2 = compressed.TrainableGroupedCompressedDense(d1, d2, gr, _dev_labels(lab2, 0), _cuda(cen2), None, None, None, half_inputs=True)
    xt = _half(x, dt, False).requires_grad_(True)
    l2(l1(xt)).backward(_half(gy, dt, False))
    c1 = torch.from_numpy(cen1).double().requires_grad_(True)
    c2 = torch.from_numpy(cen2).double().requires_grad_(True)
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    w1 = c1[torch.arange(d0)[:, None] // gr, torch.from_numpy(lab1)]
    w2 = c2[torch.arange(d1)[:, None] // gr, torch.from_numpy(lab2)]
    (torch.relu(x64 @ w1) @ w2).backward(torch.from_numpy(gy).double())
    # every product and sum is an exact float32; what the half chain rounds is what it stores in dt (y1, dL/dy1, x.grad), each once
    dx, dc1, dc2 = _chain_ref(x, lab1, lab2, cen1, cen2, gy, gr, dt)
    assert np.array_equal(l2.centers.grad.cpu().numpy().astype(np.float64), dc2)
    assert np.array_equal(l1.centers.grad.cpu().numpy().astype(np.float64), dc1)
    assert np.array_equal(xt.grad.float().cpu().numpy().astype(np.float64), dx)
    if dt == "fp16":   # 11 significant bits hold every intermediate: the rounded chain is the float64 chain
        assert np.array_equal(l1.centers.grad.cpu().numpy().astype(np.float64), c1.grad.numpy())
        assert np.array_equal(l2.centers.grad.cpu().numpy().astype(np.float64), c2.grad.numpy())


def _chain_ref(x, lab1, lab2, cen1, cen2, gy, gr, dt):
    """The two-layer chain in float64 with the one rounding the half chain makes visible: y1 and dL/dy1 stored in dt (x.grad too)."""
    from tests.helpers.h16_ref import round_to

    d0, d1 = lab1.shape
    w1 = cen1.astype(np.float64)[np.arange(d0)[:, None] // gr, lab1]
    w2 = cen2.astype(np.float64)[np.arange(d1)[:, None] // gr, lab2]
    x = x.astype(np.float64)
    y1 = round_to(np.maximum(x @ w1, 0.0), dt).astype(np.float64)
    g2 = gy.astype(np.float64)
    dc2 = np.stack([np.bincount(lab2[q * gr:(q + 1) * gr].ravel(), weights=(y1.T @ g2)[q * gr:(q + 1) * gr].ravel(), minlength=cen2.shape[1])
                    for q in range(cen2.shape[0])])
    g1 = round_to(g2 @ w2.T, dt).astype(np.float64) * (y1 > 0)
    dc1 = np.stack([np.bincount(lab1[q * gr:(q + 1) * gr].ravel(), weights=(x.T @ g1)[q * gr:(q + 1) * gr].ravel(), minlength=cen1.shape[1])
                    for q in range(cen1.shape[0])])
    dx = round_to(g1 @ w1.T, dt).astype(np.float64)
    return dx, dc1, dc2


# ------------------------------------------------------------------ the trainer
def _trainer(seed=0):
    from neural_network_compression_amd import synth
    from neural_network_compression_amd.common import trainer as tr
    from neural_network_compression_amd.le_net_300_100_trainer import LeNet300100Trainer

    tr.Trainer.pruned_indexes_by_layer.clear()
    torch.manual_seed(seed)
    t = LeNet300100Trainer()
    layers = [layer for layer in t.neural_network.get_config().values() if layer.get_weights()]
    for li, ((_, wshape, bshape), layer) in enumerate(zip(synth.LENET_300_100, layers)):
        layer.set_weights([torch.from_numpy(synth.weights(wshape, 2000 + 2 * li)).cuda(), torch.from_numpy(synth.weights(bshape, 2001 + 2 * li)).cuda()])
    rng = np.random.RandomState(1)
    x = rng.rand(512, 784).astype(np.float32)
    y = np.eye(10, dtype=np.float32)[rng.randint(0, 10, size=512)]
    return t, tr.LeNetDataset(x, y), tr.LeNetDataset(x[:128], y[:128].argmax(1)), x, y


@pytest.mark.parametrize("packed", [False, True], ids=["byte", "packed"])
def test_one_bf16_batch_of_fine_tune_grouped_is_the_step_of_the_half_network(env, packed):
    """One batch of 512: the tuned (G, K) of every layer are c - lr * grad, grad from one forward and backward of the half network
    built by hand (whose backward is the ops calls, see above), bit for bit; the write-back reaches the GroupedModel and the float
    kernel; learning_rate = 0 moves nothing; the ValueError paths."""
    ops, _ = env
    from neural_network_compression_amd import compressed
    from neural_network_compression_amd.common import trainer as tr

    LR, dt = 1e-2, torch.bfloat16
    t, data, test, x, y = _trainer()
    t.quantize(test, False, 4, "linear", group_rows=32)
    models = t.quantized_models_by_layer
    cfg = t.neural_network.get_config()
    names = [n for n, layer in cfg.items() if models.get(layer)]
    net = compressed.compress_network_trainable_grouped(t.neural_network, models, packed=packed, half_inputs=True)
    kind = compressed.TrainableGroupedPackedCompressedDense if packed else compressed.TrainableGroupedCompressedDense
    for n in names:
        assert isinstance(getattr(net, n), kind) and getattr(net, n).half_inputs
    for p in net.parameters():
        p.requires_grad_(False)
    params = {}
    for n in names:
        for key in ("centers", "bias_centers"):
            p = getattr(getattr(net, n), key)
            if p is not None:
                params[(n, key)] = p.requires_grad_(True)
    torch.manual_seed(7)
    perm = torch.randperm(512, device="cuda")                    # the one batch of the epoch: the trainer's windowed shuffle of 512 rows
    xb, yb = torch.from_numpy(x).cuda()[perm], torch.from_numpy(y).cuda()[perm]
    t._get_error(xb, yb, tr._HalfActivations(net, dt)).backward()
    want = {key: (p.detach() - LR * p.grad) for key, p in params.items()}
    assert all(p.grad.dtype == torch.float32 and bool(p.grad.abs().sum() > 0) for p in params.values())
    before = {n: models[cfg[n]][0].cluster_centers_.copy() for n in names}

    assert t.fine_tune_grouped(data, test, epochs=1, learning_rate=0.0, packed=packed, activation_dtype=dt) is not None
    for n in names:
        assert np.array_equal(models[cfg[n]][0].cluster_centers_, before[n])
    torch.manual_seed(7)
    acc = t.fine_tune_grouped(data, test, epochs=1, learning_rate=LR, packed=packed, activation_dtype=dt)
    assert len(acc) == 1 and 0.0 <= acc[0] <= 1.0
    for n in names:
        wm = models[cfg[n]][0]
        got = torch.from_numpy(np.ascontiguousarray(wm.cluster_centers_, dtype=np.float32)).cuda()
        assert _same(got, want[(n, "centers")]) and not np.array_equal(wm.cluster_centers_, before[n])
        for q, gm in enumerate(wm.models):                                       # each group's own entries, and the float kernel re-decoded
            size = int(gm.cluster_centers_.size)
            assert np.array_equal(gm.cluster_centers_.ravel(), wm.cluster_centers_[q, :size])
        parts = [ops.gather(torch.from_numpy(np.ascontiguousarray(gm.cluster_centers_.ravel(), dtype=np.float32)).cuda(), gm.labels_compact_) for gm in wm.models]
        assert torch.equal(cfg[n].kernel, torch.cat(parts).view(cfg[n].kernel.shape))
    with pytest.raises(ValueError, match="activation_dtype"):
        t.fine_tune_grouped(data, test, epochs=1, activation_dtype=torch.float64)
    with pytest.raises(ValueError, match="packed must be"):
        t.fine_tune_grouped(data, test, epochs=1, packed="yes", activation_dtype=dt)
    real = compressed.compress_network_trainable_grouped             # a layer with weights that takes no half input: fine_tune_compressed's error
    compressed.compress_network_trainable_grouped = lambda net_, models_, packed=False, half_inputs=False: real(net_, models_, packed=packed)
    try:
        with pytest.raises(ValueError, match="built with half_inputs"):
            t.fine_tune_grouped(data, test, epochs=1, packed=packed, activation_dtype=dt)
    finally:
        compressed.compress_network_trainable_grouped = real
