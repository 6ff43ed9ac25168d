"""The backward pass of the group-wise codebook matmul (nnc_cbmm_grouped_dx_f32 / nnc_cbmm_grouped_dc_f32, csrc/
nnc_cbgrad_grouped.hip) and the autograd Function ops.grouped_codebook_linear (run with -m gpu).

Exact data gives the float64 formulas bit for bit.  On float data every group's columns of dx equal codebook_matmul_dx with that
group's table, and dc equals codebook_centroid_grad on the 16-bit labels q * K + label, both bit for bit: the plans are the
ungrouped ones (tests/test_grouped_codebook_grad_abi.py).  Everything stays within the float32 bounds of DESIGN.md section 12."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import grouped_grad_ref as ref  # noqa: E402

IDS = [ref.case_id(c) for c in ref.CASES]
ALL_IDS = [ref.case_id(c) for c in ref.ALL_CASES]


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, ops

    _native.load()
    _, cus = ops.device_info()
    return ops, cus


def _dev_labels(lab, off, dtype=np.uint8):
    """The indices starting ``off`` elements into a buffer with 16 spare bytes after them."""
    host = np.ascontiguousarray(lab.astype(dtype)).ravel()
    if dtype == np.uint16:
        host = host.view(np.int16)
    buf = torch.zeros(off + host.size + 16, dtype=torch.uint8 if dtype == np.uint8 else torch.int16, device="cuda")
    buf[off: off + host.size] = torch.from_numpy(host).cuda()
    return buf[off: off + host.size]


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _dims(c):
    return c["m"], c["kdim"], c["ncols"], c["k"], c["group_rows"]


@pytest.fixture(scope="module")
def float_runs(env):
    """Every case once on float data, with and without indices beyond K: the inputs and the grouped results (left unchanged)."""
    ops, _ = env
    runs = {}

    def run(case, oob):
        key = (ref.case_id(case), oob)
        if key not in runs:
            m, kdim, ncols, k, gr = _dims(case)
            lab = ref.labels_of(case, seed=kdim + ncols, oob=oob)
            x, g, cen = ref.float_data(case, seed=m)
            labels = _dev_labels(lab, case["off"])
            xt, gt, ct = _cuda(x), _cuda(g), _cuda(cen)
            dx = ops.grouped_codebook_matmul_dx(gt, labels, ct, kdim, ncols, gr)
            dc = ops.grouped_codebook_centroid_grad(xt, gt, labels, k, kdim, ncols, gr)
            dc32 = ops.grouped_codebook_centroid_grad(xt, gt, labels, k, kdim, ncols, gr, dtype=torch.float32)
            runs[key] = dict(lab=lab, x=x, g=g, cen=cen, labels=labels, xt=xt, gt=gt, ct=ct, dx=dx, dc=dc, dc32=dc32)
        return runs[key]

    return run


@pytest.mark.parametrize("case", ref.ALL_CASES, ids=ALL_IDS)
def test_exact_data_matches_float64_bit_for_bit(env, case):
    ops, _ = env
    m, kdim, ncols, k, gr = _dims(case)
    G = ref.groups_of(case)
    lab = ref.labels_of(case, seed=3 * m + kdim, oob=k < 254)
    x, g, cen = ref.exact_data(case, seed=m + ncols)
    labels, xt, gt, ct = _dev_labels(lab, case["off"]), _cuda(x), _cuda(g), _cuda(cen)
    dx = ops.grouped_codebook_matmul_dx(gt, labels, ct, kdim, ncols, gr)
    dc = ops.grouped_codebook_centroid_grad(xt, gt, labels, k, kdim, ncols, gr)
    dc32 = ops.grouped_codebook_centroid_grad(xt, gt, labels, k, kdim, ncols, gr, dtype=torch.float32)
    assert dx.shape == (m, kdim) and dx.dtype == torch.float32
    assert dc.shape == dc32.shape == (G, k) and dc.dtype == torch.float64 and dc32.dtype == torch.float32
    want_dc = ref.dc64(case, x, g, lab)
    assert np.array_equal(dx.cpu().numpy(), ref.dx64(case, g, lab, cen))
    assert np.array_equal(dc.cpu().numpy(), want_dc)
    assert np.array_equal(dc32.cpu().numpy(), want_dc.astype(np.float32))


@pytest.mark.parametrize("oob", [False, True], ids=["inK", "beyondK"])
@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_dx_equals_the_ungrouped_kernel_group_by_group(env, float_runs, case, oob):
    ops, _ = env
    m, kdim, ncols, k, gr = _dims(case)
    r = float_runs(case, oob)
    got = r["dx"]
    for q in range(ref.groups_of(case)):
        rows = ref.group_rows_of(case, q)
        one = ops.codebook_matmul_dx(r["gt"], r["labels"], r["ct"][q].contiguous(), kdim, ncols)
        assert torch.equal(got[:, rows], one[:, rows]), q


def _dc_identity_applies(case, oob):
    return not oob and ref.groups_of(case) * case["k"] <= 1040


def test_the_dc_identity_leaves_out_two_kinds_of_case_only():
    for case in ref.CASES:
        for oob in (False, True):
            if not _dc_identity_applies(case, oob):
                assert oob or (case["k"] == 256 and ref.groups_of(case) > 1)
    assert any(_dc_identity_applies(c, False) and ref.groups_of(c) > 1 for c in ref.STREAM_CASES)
    assert any(_dc_identity_applies(c, False) and ref.groups_of(c) > 1 for c in ref.TILED_CASES)


@pytest.mark.parametrize("case", [c for c in ref.CASES if _dc_identity_applies(c, False)],
                         ids=[ref.case_id(c) for c in ref.CASES if _dc_identity_applies(c, False)])
def test_dc_equals_the_ungrouped_kernel_on_16_bit_labels(env, float_runs, case):
    ops, _ = env
    m, kdim, ncols, k, gr = _dims(case)
    r = float_runs(case, False)
    gk = ref.groups_of(case) * k
    lab16 = _dev_labels(ref.labels16(case, r["lab"]), 0, dtype=np.uint16)
    for dt, got in ((torch.float64, r["dc"]), (torch.float32, r["dc32"])):
        want = ops.codebook_centroid_grad(r["xt"], r["gt"], lab16, gk, kdim, ncols, dtype=dt)
        assert torch.equal(got.reshape(-1), want), dt


@pytest.mark.parametrize("oob", [False, True], ids=["inK", "beyondK"])
@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_float_data_is_within_the_float32_bounds(env, float_runs, case, oob):
    ops, cus = env
    m, kdim, ncols, k, gr = _dims(case)
    r = float_runs(case, oob)
    lab, x, g, cen = r["lab"], r["x"], r["g"], r["cen"]
    dx = r["dx"].cpu().numpy().astype(np.float64)
    assert np.all(np.abs(dx - ref.dx64(case, g, lab, cen)) <= ref.dx_bound(case, g, lab, cen))
    t = ops.cbmm_grouped_dc_plan(m, kdim, ncols, k, gr, cus)["terms_log2"]
    S, flag = ops.cbgrad_shift(m, np.abs(x).max(), np.abs(g).max(), t)
    assert flag == ops.CBGRAD_OK
    want = ref.dc64(case, x, g, lab)
    for got, f32 in ((r["dc"], False), (r["dc32"], True)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        assert np.all(err <= ref.dc_bound(case, x, g, lab, S, f32_out=f32))


@pytest.mark.parametrize("case", ref.ONE_GROUP_CASES + ref.SHORT_CASES, ids=[ref.case_id(c) for c in ref.ONE_GROUP_CASES + ref.SHORT_CASES])
def test_one_group_equals_the_ungrouped_calls(env, float_runs, case):
    ops, _ = env
    m, kdim, ncols, k, gr = _dims(case)
    assert ref.groups_of(case) == 1
    for oob in (False, True):
        r = float_runs(case, oob)
        assert torch.equal(r["dx"], ops.codebook_matmul_dx(r["gt"], r["labels"], r["ct"][0].contiguous(), kdim, ncols))
        assert torch.equal(r["dc"][0], ops.codebook_centroid_grad(r["xt"], r["gt"], r["labels"], k, kdim, ncols))
        assert torch.equal(r["dc32"][0], ops.codebook_centroid_grad(r["xt"], r["gt"], r["labels"], k, kdim, ncols, dtype=torch.float32))


@pytest.mark.parametrize("case", ref.CASES, ids=IDS)
def test_two_calls_give_the_same_bits(env, float_runs, case):
    ops, _ = env
    m, kdim, ncols, k, gr = _dims(case)
    r = float_runs(case, True)
    assert torch.equal(ops.grouped_codebook_matmul_dx(r["gt"], r["labels"], r["ct"], kdim, ncols, gr), r["dx"])
    assert torch.equal(ops.grouped_codebook_centroid_grad(r["xt"], r["gt"], r["labels"], k, kdim, ncols, gr), r["dc"])


def test_non_finite_and_zero_inputs(env):
    ops, _ = env
    case = ref.STREAM_CASES[0]
    m, kdim, ncols, k, gr = _dims(case)
    lab = ref.labels_of(case, 5)
    x, g, cen = ref.exact_data(case, 5)
    labels = _dev_labels(lab, 0)
    for mm in (m, 17):
        xx, gg = np.resize(x, (mm, kdim)).copy(), np.resize(g, (mm, ncols)).copy()
        assert (ops.grouped_codebook_centroid_grad(_cuda(xx * 0), _cuda(gg), labels, k, kdim, ncols, gr) == 0).all()
        xx[1, 5] = np.inf
        assert torch.isnan(ops.grouped_codebook_centroid_grad(_cuda(xx), _cuda(gg), labels, k, kdim, ncols, gr)).all()
        xx[1, 5] = 3e38                                        # m * max|x| * max|g| >= 2^127: P > 127
        gg[0, 0] = 3e38
        assert torch.isnan(ops.grouped_codebook_centroid_grad(_cuda(xx), _cuda(gg), labels, k, kdim, ncols, gr)).all()


# ------------------------------------------------------------------ autograd
KD, NC, K, GR = 90, 150, 12, 32


def _layer(m, seed=0):
    rng = np.random.RandomState(seed)
    G = -(-KD // GR)
    x = rng.randint(-3, 4, size=(m, KD)).astype(np.float32)
    cen = (rng.randint(-8, 9, size=(G, K)) / 4.0 + 8.0 * np.arange(G)[:, None]).astype(np.float32)
    lab = rng.randint(0, K, size=(KD, NC))
    b = (rng.randint(-5, 6, size=NC) - 300 * (np.arange(NC) % 2)).astype(np.float32)   # (half of the outputs below zero for the ReLU)
    return x, cen, lab, b


@pytest.mark.parametrize("m", [5, 40])
def test_grouped_codebook_linear_no_grad_equals_grouped_codebook_matmul(env, m):
    ops, _ = env
    x, cen, lab, b = _layer(m)
    xt = (_cuda(x) * 0.37).requires_grad_(True)
    ct, bt, labels = _cuda(cen).requires_grad_(True), _cuda(b).requires_grad_(True), _dev_labels(lab, 1)
    for relu in (False, True):
        with torch.no_grad():
            y = ops.grouped_codebook_linear(xt, labels, ct, KD, NC, GR, bias=bt, relu=relu)
            want = ops.grouped_codebook_matmul(xt, labels, ct, KD, NC, GR, bias=bt, relu=relu)
        assert torch.equal(y, want)


@pytest.mark.parametrize("m", [5, 40])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("bias", [False, True])
def test_grouped_codebook_linear_matches_torch_autograd_in_float64(env, m, relu, bias):
    ops, _ = env
    x, cen, lab, b = _layer(m, seed=m)
    gy = np.random.RandomState(m + 1).randint(-3, 4, size=(m, NC)).astype(np.float32)
    xt, ct = _cuda(x).requires_grad_(True), _cuda(cen).requires_grad_(True)
    bt = _cuda(b).requires_grad_(True) if bias else None
    y = ops.grouped_codebook_linear(xt, _dev_labels(lab, 0), ct, KD, NC, GR, bias=bt, relu=relu)
    y.backward(_cuda(gy))
    # torch autograd on W = table[group, labels] in float64
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
    y = ops.grouped_codebook_linear(xt, _dev_labels(lab, 0), ct, KD, NC, GR, bias=_cuda(b), relu=True)
    yh = y.detach().cpu().numpy()
    assert np.isnan(yh[0]).all() and (yh[1:] == 0).any() and (yh[1:] > 0).any()
    y.backward(torch.ones_like(y))
    assert (xt.grad[0] == 0).all() and not torch.isnan(xt.grad).any()


def test_only_the_needed_kernels_run(env, monkeypatch):
    ops, _ = env
    x, cen, lab, b = _layer(3)
    labels = _dev_labels(lab, 0)
    calls = []
    real_dx, real_dc = ops.grouped_codebook_matmul_dx, ops.grouped_codebook_centroid_grad
    monkeypatch.setattr(ops, "grouped_codebook_matmul_dx", lambda *a, **k: calls.append("dx") or real_dx(*a, **k))
    monkeypatch.setattr(ops, "grouped_codebook_centroid_grad", lambda *a, **k: calls.append("dc") or real_dc(*a, **k))
    ops.grouped_codebook_linear(_cuda(x).requires_grad_(True), labels, _cuda(cen), KD, NC, GR).sum().backward()
    assert calls == ["dx"]
    calls.clear()
    ops.grouped_codebook_linear(_cuda(x), labels, _cuda(cen).requires_grad_(True), KD, NC, GR).sum().backward()
    assert calls == ["dc"]
    calls.clear()
    ops.grouped_codebook_linear(_cuda(x), labels, _cuda(cen), KD, NC, GR, bias=_cuda(b).requires_grad_(True)).sum().backward()
    assert calls == []


def test_forward_and_backward_read_nothing_back(env):
    ops, _ = env
    x, cen, lab, b = _layer(16)
    xt, ct, bt = _cuda(x).requires_grad_(True), _cuda(cen).requires_grad_(True), _cuda(b).requires_grad_(True)
    labels = _dev_labels(lab, 0)
    x40 = xt[:5].detach().repeat(8, 1).requires_grad_(True)
    g16, g40 = torch.ones(16, NC, device="cuda"), torch.ones(40, NC, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for relu in (False, True):
            ops.grouped_codebook_linear(xt, labels, ct, KD, NC, GR, bias=bt, relu=relu).backward(g16)
            ops.grouped_codebook_linear(x40, labels, ct, KD, NC, GR, relu=relu).backward(g40)
    finally:
        torch.cuda.set_sync_debug_mode(0)


def test_backward_memory_is_outputs_plus_workspace(env):
    ops, cus = env
    kdim = ncols = 4096
    k, gr, m = 16, 128, 16
    G = kdim // gr
    labels = torch.randint(0, k, (kdim * ncols,), dtype=torch.uint8, device="cuda")
    ct = (torch.randn(G, k, device="cuda") * 0.1).requires_grad_(True)
    xt = torch.randn(m, kdim, device="cuda").requires_grad_(True)
    y = ops.grouped_codebook_linear(xt, labels, ct, kdim, ncols, gr)
    gy = torch.randn_like(y)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    y.backward(gy)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    ws = ops.cbmm_grouped_dx_plan(m, kdim, ncols, k, gr, cus)["workspace"] + ops.cbmm_grouped_dc_plan(m, kdim, ncols, k, gr, cus)["workspace"]
    outputs = m * kdim * 4 + G * k * 4
    assert growth <= outputs + ws + (1 << 20), (growth, outputs, ws)
    assert growth < kdim * ncols * 4 // 4


def test_argument_errors(env):
    ops, _ = env
    from neural_network_compression_amd import _native as nat

    x, cen, lab, b = _layer(4)
    xt, ct, labels = _cuda(x), _cuda(cen), _dev_labels(lab, 0)
    gt = torch.ones(4, NC, device="cuda")
    with pytest.raises(TypeError, match="float32 activations"):
        ops.grouped_codebook_linear(xt.half(), labels, ct, KD, NC, GR)
    with pytest.raises(TypeError, match="uint8"):
        ops.grouped_codebook_linear(xt, labels.to(torch.int16), ct, KD, NC, GR)
    with pytest.raises(TypeError, match="uint8"):
        ops.grouped_codebook_matmul_dx(gt, labels.to(torch.int16), ct, KD, NC, GR)
    with pytest.raises(TypeError, match="uint8"):
        ops.grouped_codebook_centroid_grad(xt, gt, labels.to(torch.int16), K, KD, NC, GR)
    for bad in (0, 16, 48, -32):
        with pytest.raises(ValueError, match="group_rows"):
            ops.grouped_codebook_matmul_dx(gt, labels, ct, KD, NC, bad)
        with pytest.raises(ValueError, match="group_rows"):
            ops.grouped_codebook_centroid_grad(xt, gt, labels, K, KD, NC, bad)
    for shape in (ct[:2].contiguous(), ct.reshape(-1), torch.zeros(3, 257, device="cuda")):
        with pytest.raises(ValueError, match="centers must have shape"):
            ops.grouped_codebook_matmul_dx(gt, labels, shape, KD, NC, GR)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="one device"):
            ops.grouped_codebook_matmul_dx(gt, labels, ct.to("cuda:1"), KD, NC, GR)
        with pytest.raises(ValueError, match="one device"):
            ops.grouped_codebook_centroid_grad(xt.to("cuda:1"), gt, labels, K, KD, NC, GR)
    with pytest.raises(TypeError, match="CUDA"):              # (and a host tensor is no operand at all)
        ops.grouped_codebook_matmul_dx(gt, labels, ct.cpu(), KD, NC, GR)
    L = nat.load()
    assert L.nnc_cbmm_grouped_dx_f32(gt.data_ptr(), 4, KD, labels.data_ptr(), NC, ct.data_ptr(), K, 48, xt.data_ptr(), None, 0, None) == -1
    assert L.nnc_cbmm_grouped_dc_f32(xt.data_ptr(), gt.data_ptr(), 4, KD, labels.data_ptr(), NC, 257, GR, ct.data_ptr(), 0, None, 0, None) == -1

