"""The backward pass of the group-wise codebook matmul on 2- and 4-bit packed indices (nnc_cbpk_grouped_dx_f32 /
nnc_cbpk_grouped_dc_f32, csrc/nnc_cbpkgrad_grouped.hip) and the autograd Function
ops.grouped_packed_codebook_linear (run with -m gpu).

Exact data gives the float64 formulas bit for bit.  On float data three identities hold bit for bit, because the plans are the
ungrouped packed ones (tests/test_grouped_packed_codebook_grad_abi.py): (A) every group's columns of dx equal
packed_codebook_matmul_dx with that group's table; (B) dc equals grouped_codebook_centroid_grad on the unpacked labels; (C) with one
group both calls equal the ungrouped packed ones.  dx stays within the derived float32 bound of DESIGN.md section 12."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import grouped_packed_grad_ref as ref  # noqa: E402
from tests.helpers import packed_grad_ref  # noqa: E402

IDS = [ref.case_id(c) for c in ref.CASES]
ALL_IDS = [ref.case_id(c) for c in ref.ALL_CASES]


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, ops

    _native.load()
    _, cus = ops.device_info()
    return ops, cus


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dims(c):
    return c["m"], c["kdim"], c["ncols"], c["bits"], c["k"], c["group_rows"]


def _codes(ops, lab, bits, k):
    kdim, ncols = lab.shape
    return ops.pack_codes(torch.from_numpy(np.ascontiguousarray(lab, dtype=np.uint8).ravel()).cuda(), kdim, ncols, k, bits)


@pytest.fixture(scope="module")
def float_runs(env):
    """Every case once on float data, labels up to 2^bits - 1: the inputs and the grouped packed results (left unchanged)."""
    ops, _ = env
    runs = {}

    def run(case):
        key = ref.case_id(case)
        if key not in runs:
            m, kdim, ncols, bits, k, gr = _dims(case)
            lab = ref.labels_of(case, seed=kdim + ncols + bits)
            x, g, cen = ref.float_data(case, seed=m)
            codes = _codes(ops, lab, bits, k)
            xt, gt, ct = _cuda(x), _cuda(g), _cuda(cen)
            dx = ops.grouped_packed_codebook_matmul_dx(gt, codes, ct, gr)
            dc = ops.grouped_packed_codebook_centroid_grad(xt, gt, codes, gr)
            dc32 = ops.grouped_packed_codebook_centroid_grad(xt, gt, codes, gr, dtype=torch.float32)
            runs[key] = dict(lab=lab, x=x, g=g, cen=cen, codes=codes, xt=xt, gt=gt, ct=ct, dx=dx, dc=dc, dc32=dc32)
        return runs[key]

    return run


@pytest.mark.parametrize("case", ref.ALL_CASES, ids=ALL_IDS)
def test_exact_data_matches_float64_bit_for_bit(env, case):
    ops, _ = env
    m, kdim, ncols, bits, k, gr = _dims(case)
    G = ref.groups_of(case)
    lab = ref.labels_of(case, seed=3 * m + kdim)
    x, g, cen = ref.exact_data(case, seed=m + ncols)
    codes, xt, gt, ct = _codes(ops, lab, bits, k), _cuda(x), _cuda(g), _cuda(cen)
    dx = ops.grouped_packed_codebook_matmul_dx(gt, codes, ct, gr)
    dc = ops.grouped_packed_codebook_centroid_grad(xt, gt, codes, gr)
    dc32 = ops.grouped_packed_codebook_centroid_grad(xt, gt, codes, gr, dtype=torch.float32)
    assert dx.shape == (m, kdim) and dx.dtype == torch.float32
    assert dc.shape == dc32.shape == (G, k) and dc.dtype == torch.float64 and dc32.dtype == torch.float32
    want_dc = ref.dc64(case, x, g, lab)
    assert np.array_equal(dx.cpu().numpy(), ref.dx64(case, g, lab, cen))
    assert np.array_equal(dc.cpu().numpy(), want_dc)
    assert np.array_equal(dc32.cpu().numpy(), want_dc.astype(np.float32))
    assert torch.equal(dx, ops.grouped_codebook_matmul_dx(gt, codes.to_dense(), ct, kdim, ncols, gr))


@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_identity_a_dx_equals_the_ungrouped_packed_kernel_group_by_group(env, float_runs, case):
    ops, _ = env
    r = float_runs(case)
    if case["k"] < (1 << case["bits"]):
        assert (r["lab"] >= case["k"]).any()
    for q in range(ref.groups_of(case)):
        rows = ref.group_rows_of(case, q)
        one = ops.packed_codebook_matmul_dx(r["gt"], r["codes"], r["ct"][q].contiguous())
        assert torch.equal(r["dx"][:, rows], one[:, rows]), q


@pytest.mark.parametrize("case", ref.ALL_CASES, ids=ALL_IDS)
def test_identity_b_dc_equals_the_grouped_byte_kernel(env, float_runs, case):
    ops, _ = env
    m, kdim, ncols, bits, k, gr = _dims(case)
    r = float_runs(case)
    labels = r["codes"].to_dense()
    for dt, got in ((torch.float64, r["dc"]), (torch.float32, r["dc32"])):
        want = ops.grouped_codebook_centroid_grad(r["xt"], r["gt"], labels, k, kdim, ncols, gr, dtype=dt)
        assert got.dtype == dt and torch.equal(got, want), dt


ONE_GROUP = ref.ONE_GROUP_CASES + ref.SHORT_CASES + [dict(c, group_rows=32 * max(1, -(-c["kdim"] // 32))) for c in ref.PACKED_CASES if c["m"] * c["kdim"] * c["ncols"]]


@pytest.mark.parametrize("case", ONE_GROUP, ids=[ref.case_id(c) for c in ONE_GROUP])
def test_identity_c_one_group_equals_the_ungrouped_packed_calls(env, float_runs, case):
    ops, _ = env
    assert ref.groups_of(case) == 1 and case["group_rows"] >= case["kdim"]
    r = float_runs(case)
    c0 = r["ct"][0].contiguous()
    assert torch.equal(r["dx"], ops.packed_codebook_matmul_dx(r["gt"], r["codes"], c0))
    assert torch.equal(r["dc"][0], ops.packed_codebook_centroid_grad(r["xt"], r["gt"], r["codes"]))
    assert torch.equal(r["dc32"][0], ops.packed_codebook_centroid_grad(r["xt"], r["gt"], r["codes"], dtype=torch.float32))


@pytest.mark.parametrize("case,want", list(zip(ref.WIDE_CASES, ref.WIDE_EXPECT)), ids=[ref.case_id(c) for c in ref.WIDE_CASES])
def test_the_wide_instantiations_hold_the_identities(env, case, want):
    """The 8- and 16-byte loads are planned for large layers only: identities (A) and (B) on device-made data, no float64 reference."""
    ops, cus = env
    m, kdim, ncols, bits, k, gr = _dims(case)
    plan = ops.cbpk_grouped_dx_plan(m, kdim, ncols, bits, k, gr, cus)
    assert (bits, plan["vb"], plan["mt"]) == want and plan["groups"] == 3
    gen = torch.Generator(device="cuda").manual_seed(kdim + ncols + m)
    labels = torch.randint(0, 1 << bits, (kdim * ncols,), dtype=torch.uint8, device="cuda", generator=gen)
    codes = ops.pack_codes(labels, kdim, ncols, k, bits)
    G = ref.groups_of(case)
    ct = torch.randn(G, k, device="cuda", generator=gen) + 64.0 * torch.arange(G, device="cuda")[:, None]
    xt = torch.randn(m, kdim, device="cuda", generator=gen)
    gt = torch.randn(m, ncols, device="cuda", generator=gen) * 1e-2
    dx = ops.grouped_packed_codebook_matmul_dx(gt, codes, ct, gr)
    for q in range(G):
        rows = ref.group_rows_of(case, q)
        assert torch.equal(dx[:, rows], ops.packed_codebook_matmul_dx(gt, codes, ct[q].contiguous())[:, rows]), q
    for dt in (torch.float64, torch.float32):
        dc = ops.grouped_packed_codebook_centroid_grad(xt, gt, codes, gr, dtype=dt)
        assert torch.equal(dc, ops.grouped_codebook_centroid_grad(xt, gt, labels, k, kdim, ncols, gr, dtype=dt))
        assert torch.equal(dc, ops.grouped_packed_codebook_centroid_grad(xt, gt, codes, gr, dtype=dt))


@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_float_data_is_within_the_float32_bounds(env, float_runs, case):
    ops, cus = env
    m, kdim, ncols, bits, k, gr = _dims(case)
    r = float_runs(case)
    lab, x, g, cen = r["lab"], r["x"], r["g"], r["cen"]
    dx = r["dx"].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(dx - ref.dx64(case, g, lab, cen)) <= ref.dx_bound(case, g, lab, cen))
    t = ops.cbpk_grouped_dc_plan(m, kdim, ncols, bits, k, gr, cus)["terms_log2"]
    S, flag = ops.cbgrad_shift(m, np.abs(x).max(), np.abs(g).max(), t)
    assert flag == ops.CBGRAD_OK
    want = ref.dc64(case, x, g, lab)
    for got, f32 in ((r["dc"], False), (r["dc32"], True)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        assert np.all(err <= ref.dc_bound(case, x, g, lab, S, f32_out=f32))


def _tail(host):
    """A contiguous view that ends where its allocation ends, NaN in front of it."""
    host = np.ascontiguousarray(host, dtype=np.float32)
    buf = torch.full((host.size + 3,), float("nan"), dtype=torch.float32, device="cuda")
    buf[3:] = torch.from_numpy(host.ravel()).cuda()
    return buf[3:].view(host.shape)


@pytest.mark.parametrize("m", [2, 16, 17])
@pytest.mark.parametrize("ncols,bits,k", [(48, 4, 16), (50, 2, 4), (7, 4, 3), (1027, 2, 3)])
def test_padding_is_neither_a_weight_nor_binned(env, m, ncols, bits, k):
    """Rows that leave padding; only the padding fields hold label 0.  Whatever centers[:, 0] is, dx does not change and bin 0 of
    every group stays empty; g ends where its allocation ends, so a lane past ncols has nothing to load."""
    ops, _ = env
    case = dict(m=m, kdim=112, ncols=ncols, bits=bits, k=k, group_rows=32, off=0)
    assert ncols * bits % 128 != 0
    rng = np.random.RandomState(100 * m + ncols)
    lab = rng.randint(1, 1 << bits, size=(112, ncols))
    x, g, cen = ref.exact_data(case, seed=m)
    codes = _codes(ops, lab, bits, k)
    xt, gt = _tail(x), _tail(g)
    big = cen.copy()
    big[:, 0] = 3e38
    dx = ops.grouped_packed_codebook_matmul_dx(gt, codes, _cuda(cen), 32)
    dx_big = ops.grouped_packed_codebook_matmul_dx(gt, codes, _cuda(big), 32)
    assert torch.isfinite(dx_big).all() and torch.equal(dx, dx_big)
    assert np.array_equal(dx.cpu().numpy(), ref.dx64(case, g, lab, cen))
    for dt in (torch.float64, torch.float32):
        dc = ops.grouped_packed_codebook_centroid_grad(xt, gt, codes, 32, dtype=dt)
        assert (dc[:, 0] == 0).all()
        assert np.array_equal(dc.cpu().numpy(), ref.dc64(case, x, g, lab).astype(dc.cpu().numpy().dtype))


@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_two_calls_give_the_same_bits(env, float_runs, case):
    ops, _ = env
    r = float_runs(case)
    gr = case["group_rows"]
    assert torch.equal(ops.grouped_packed_codebook_matmul_dx(r["gt"], r["codes"], r["ct"], gr), r["dx"])
    assert torch.equal(ops.grouped_packed_codebook_centroid_grad(r["xt"], r["gt"], r["codes"], gr), r["dc"])


def test_non_finite_and_zero_inputs(env):
    ops, _ = env
    case = ref.STREAM_CASES[0]
    m, kdim, ncols, bits, k, gr = _dims(case)
    lab = ref.labels_of(case, 5)
    x, g, cen = ref.exact_data(case, 5)
    codes = _codes(ops, lab, bits, k)
    for mm in (m, 17):
        xx, gg = np.resize(x, (mm, kdim)).copy(), np.resize(g, (mm, ncols)).copy()
        for dt in (torch.float64, torch.float32):
            assert (ops.grouped_packed_codebook_centroid_grad(_cuda(xx * 0), _cuda(gg), codes, gr, dtype=dt) == 0).all()
            assert (ops.grouped_packed_codebook_centroid_grad(_cuda(xx), _cuda(gg * 0), codes, gr, dtype=dt) == 0).all()
        xx[1, 5] = np.inf
        assert torch.isnan(ops.grouped_packed_codebook_centroid_grad(_cuda(xx), _cuda(gg), codes, gr)).all()
        xx[1, 5] = np.nan
        assert torch.isnan(ops.grouped_packed_codebook_centroid_grad(_cuda(xx), _cuda(gg), codes, gr, dtype=torch.float32)).all()
        xx[1, 5] = 3e38                                        # m * max|x| * max|g| >= 2^127: P > 127
        gg[0, 0] = 3e38
        assert torch.isnan(ops.grouped_packed_codebook_centroid_grad(_cuda(xx), _cuda(gg), codes, gr)).all()


# ------------------------------------------------------------------ autograd
KD, NC, K, GR, BITS = 90, 150, 12, 32, 4


def _layer(m, seed=0):
    rng = np.random.RandomState(seed)
    G = -(-KD // GR)
    x = rng.randint(-3, 4, size=(m, KD)).astype(np.float32)
    cen = (rng.randint(-8, 9, size=(G, K)) / 4.0 + 8.0 * np.arange(G)[:, None]).astype(np.float32)
    lab = rng.randint(0, K, size=(KD, NC))
    b = (rng.randint(-5, 6, size=NC) - 300 * (np.arange(NC) % 2)).astype(np.float32)   # (half of the outputs below zero for the ReLU)
    return x, cen, lab, b


@pytest.mark.parametrize("m", [5, 40])
def test_grouped_packed_codebook_linear_no_grad_equals_grouped_packed_codebook_matmul(env, m):
    ops, _ = env
    x, cen, lab, b = _layer(m)
    xt = (_cuda(x) * 0.37).requires_grad_(True)
    ct, bt, codes = _cuda(cen).requires_grad_(True), _cuda(b).requires_grad_(True), _codes(ops, lab, BITS, K)
    for relu in (False, True):
        with torch.no_grad():
            y = ops.grouped_packed_codebook_linear(xt, codes, ct, GR, bias=bt, relu=relu)
            want = ops.grouped_packed_codebook_matmul(xt, codes, ct, GR, bias=bt, relu=relu)
        assert torch.equal(y, want)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.grouped_packed_codebook_matmul(xt, codes, ct, GR)


@pytest.mark.parametrize("m", [5, 40])
def test_the_centre_gradient_is_the_byte_grouped_layers_bit_for_bit(env, m):
    ops, _ = env
    x, cen, lab, b = _layer(m, seed=m)
    x = x * np.float32(0.37)
    gy = _cuda((np.random.RandomState(m).standard_normal((m, NC)) * 1e-2).astype(np.float32))
    codes = _codes(ops, lab, BITS, K)
    grads = []
    for form in ("packed", "byte"):
        xt, ct = _cuda(x).requires_grad_(True), _cuda(cen).requires_grad_(True)
        if form == "packed":
            y = ops.grouped_packed_codebook_linear(xt, codes, ct, GR)
        else:
            y = ops.grouped_codebook_linear(xt, codes.to_dense(), ct, KD, NC, GR)
        y.backward(gy)
        grads.append((y.detach(), ct.grad, xt.grad))
    # (the forward sums of the two forms follow different plans at m <= 16; the centre gradient has x and the upstream gradient only)
    assert grads[0][1].dtype == torch.float32 and torch.equal(grads[0][1], grads[1][1])
    assert grads[0][2].shape == (m, KD)


@pytest.mark.parametrize("m", [5, 40])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("bias", [False, True])
def test_grouped_packed_codebook_linear_matches_torch_autograd_in_float64(env, m, relu, bias):
    """Integer x and upstream gradient, quarter-integer centres: every float32 sum is exact, so the derived dx and dc bounds of
    DESIGN.md section 12 are met with zero error, as in the byte grouped test."""
    ops, _ = env
    x, cen, lab, b = _layer(m, seed=m)
    gy = np.random.RandomState(m + 1).randint(-3, 4, size=(m, NC)).astype(np.float32)
    xt, ct = _cuda(x).requires_grad_(True), _cuda(cen).requires_grad_(True)
    bt = _cuda(b).requires_grad_(True) if bias else None
    y = ops.grouped_packed_codebook_linear(xt, _codes(ops, lab, BITS, K), ct, GR, bias=bt, relu=relu)
    y.backward(_cuda(gy))
    x64, c64 = torch.from_numpy(x).double().requires_grad_(True), torch.from_numpy(cen).double().requires_grad_(True)
    b64 = torch.from_numpy(b).double().requires_grad_(True) if bias else None
    w = c64[torch.arange(KD)[:, None] // GR, torch.from_numpy(lab)]
    y64 = x64 @ w + (b64 if bias else 0.0)
    y64 = torch.relu(y64) if relu else y64
    y64.backward(torch.from_numpy(gy).double())
    assert not torch.isnan(y).any()
    assert np.array_equal(y.detach().cpu().numpy(), y64.detach().numpy())
    assert np.array_equal(xt.grad.cpu().numpy(), x64.grad.numpy())
    assert ct.grad.shape == (cen.shape[0], K) and np.array_equal(ct.grad.cpu().numpy(), c64.grad.numpy().astype(np.float32))
    if bias:
        assert np.array_equal(bt.grad.cpu().numpy(), b64.grad.numpy())


def test_relu_gives_a_nan_output_no_gradient(env):
    ops, _ = env
    x, cen, lab, b = _layer(4, seed=9)
    x[0, 3] = np.nan
    xt, ct = _cuda(x).requires_grad_(True), _cuda(cen).requires_grad_(True)
    y = ops.grouped_packed_codebook_linear(xt, _codes(ops, lab, BITS, K), ct, GR, bias=_cuda(b), relu=True)
    yh = y.detach().cpu().numpy()
    assert np.isnan(yh[0]).all() and (yh[1:] == 0).any() and (yh[1:] > 0).any()
    y.backward(torch.ones_like(y))
    assert (xt.grad[0] == 0).all() and not torch.isnan(xt.grad).any()


def test_only_the_needed_kernels_run(env, monkeypatch):
    ops, _ = env
    x, cen, lab, b = _layer(3)
    codes = _codes(ops, lab, BITS, K)
    calls = []
    real_dx, real_dc = ops.grouped_packed_codebook_matmul_dx, ops.grouped_packed_codebook_centroid_grad
    monkeypatch.setattr(ops, "grouped_packed_codebook_matmul_dx", lambda *a, **k: calls.append("dx") or real_dx(*a, **k))
    monkeypatch.setattr(ops, "grouped_packed_codebook_centroid_grad", lambda *a, **k: calls.append("dc") or real_dc(*a, **k))
    ops.grouped_packed_codebook_linear(_cuda(x).requires_grad_(True), codes, _cuda(cen), GR).sum().backward()
    assert calls == ["dx"]
    calls.clear()
    ops.grouped_packed_codebook_linear(_cuda(x), codes, _cuda(cen).requires_grad_(True), GR).sum().backward()
    assert calls == ["dc"]
    calls.clear()
    ops.grouped_packed_codebook_linear(_cuda(x), codes, _cuda(cen), GR, bias=_cuda(b).requires_grad_(True)).sum().backward()
    assert calls == []


def test_forward_and_backward_read_nothing_back(env):
    ops, _ = env
    x, cen, lab, b = _layer(16)
    xt, ct, bt = _cuda(x).requires_grad_(True), _cuda(cen).requires_grad_(True), _cuda(b).requires_grad_(True)
    codes = _codes(ops, lab, BITS, K)
    x40 = xt[:5].detach().repeat(8, 1).requires_grad_(True)
    g16, g40 = torch.ones(16, NC, device="cuda"), torch.ones(40, NC, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for relu in (False, True):
            ops.grouped_packed_codebook_linear(xt, codes, ct, GR, bias=bt, relu=relu).backward(g16)
            ops.grouped_packed_codebook_linear(x40, codes, ct, GR, relu=relu).backward(g40)
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_backward_memory_is_outputs_plus_workspace(env):
    ops, cus = env
    kdim = ncols = 4096
    k, bits, gr, m = 16, 4, 128, 16
    G = kdim // gr
    codes = ops.pack_codes(torch.randint(0, k, (kdim * ncols,), dtype=torch.uint8, device="cuda"), kdim, ncols, k, bits)
    ct = (torch.randn(G, k, device="cuda") * 0.1).requires_grad_(True)
    xt = torch.randn(m, kdim, device="cuda").requires_grad_(True)
    y = ops.grouped_packed_codebook_linear(xt, codes, ct, gr)
    gy = torch.randn_like(y)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y.backward(gy)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    ws = (ops.cbpk_grouped_dx_plan(m, kdim, ncols, bits, k, gr, cus)["workspace"]
          + ops.cbpk_grouped_dc_plan(m, kdim, ncols, bits, k, gr, cus)["workspace"])
    outputs = m * kdim * 4 + G * k * 4
    assert growth <= outputs + ws + (1 << 20), (growth, outputs, ws)
    assert growth < kdim * ncols                 # below one byte per weight: nothing is unpacked


def test_argument_errors(env):
    ops, _ = env
    from neural_network_compression_amd import _native as nat

    x, cen, lab, b = _layer(4)
    xt, ct, codes = _cuda(x), _cuda(cen), _codes(ops, lab, BITS, K)
    gt = torch.ones(4, NC, device="cuda")
    with pytest.raises(TypeError, match="float32 activations"):
        ops.grouped_packed_codebook_linear(xt.half(), codes, ct, GR)
    with pytest.raises(TypeError, match="float32 activations"):
        ops.grouped_packed_codebook_linear(xt.bfloat16(), codes, ct, GR)
    for fn in (lambda c: ops.grouped_packed_codebook_linear(xt, c, ct, GR), lambda c: ops.grouped_packed_codebook_matmul_dx(gt, c, ct, GR),
               lambda c: ops.grouped_packed_codebook_centroid_grad(xt, gt, c, GR)):
        with pytest.raises(TypeError, match="PackedCodes"):
            fn(codes.to_dense())
    for bad in (0, 16, 48, -32):
        with pytest.raises(ValueError, match="group_rows"):
            ops.grouped_packed_codebook_matmul_dx(gt, codes, ct, bad)
        with pytest.raises(ValueError, match="group_rows"):
            ops.grouped_packed_codebook_centroid_grad(xt, gt, codes, bad)
    for shape in (ct[:2].contiguous(), ct.reshape(-1), torch.zeros(3, 16, device="cuda")):
        with pytest.raises(ValueError, match="centers must have shape"):
            ops.grouped_packed_codebook_matmul_dx(gt, codes, shape, GR)
    with pytest.raises(ValueError):
        ops.grouped_packed_codebook_matmul_dx(gt[:, :-1].contiguous(), codes, ct, GR)
    with pytest.raises(ValueError):
        ops.grouped_packed_codebook_centroid_grad(xt[:3], gt, codes, GR)
    with pytest.raises(TypeError):
        ops.grouped_packed_codebook_centroid_grad(xt, gt, codes, GR, dtype=torch.float16)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="one device"):
            ops.grouped_packed_codebook_matmul_dx(gt, codes, ct.to("cuda:1"), GR)
    with pytest.raises(TypeError, match="CUDA"):              # (and a host tensor is no operand at all)
        ops.grouped_packed_codebook_matmul_dx(gt, codes, ct.cpu(), GR)
    L = nat.load()
    pk = codes.packed
    assert L.nnc_cbpk_grouped_dx_f32(gt.data_ptr(), 4, KD, pk.data_ptr(), pk.numel(), BITS, NC, ct.data_ptr(), K, 48, xt.data_ptr(), None, 0, None) == -1
    assert L.nnc_cbpk_grouped_dx_f32(gt.data_ptr(), 4, KD, pk.data_ptr(), pk.numel() - 16, BITS, NC, ct.data_ptr(), K, GR, xt.data_ptr(), None, 0, None) == -1
    assert L.nnc_cbpk_grouped_dc_f32(xt.data_ptr(), gt.data_ptr(), 4, KD, pk.data_ptr(), pk.numel(), BITS, NC, 17, GR, ct.data_ptr(), 0, None, 0, None) == -1
