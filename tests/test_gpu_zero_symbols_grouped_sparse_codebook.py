"""The group-wise codebook layer run from the bitmap-sparse form of its indices (nnc_cbsp_grouped_*, csrc/nnc_cbsp_grouped.hip,
DESIGN.md section 28) against NumPy, through ops.pack_grouped_sparse_codes / grouped_sparse_codebook_matmul,
GroupedSparseCompressedDense, sparsify_grouped_layers and smallest_grouped_layers (run with -m gpu).

Every case of tests/helpers/grouped_sparse_ref.py: the pack against a NumPy construction of the buffer byte for byte and unpack of
pack the identity; exact data bit for bit against the float64 formula (with and without ReLU) and against
ops.grouped_codebook_matmul on the unpacked labels; float data within the derived bound
2 (kdim + 4) u (|x| @ |D| + sum_g |c_{z_g}| sum_{i in g} |x| + |b|) + u (|x| @ |C - c_z|) of the float64 product with the decoded W.
Then one group against ops.sparse_codebook_matmul (bit for bit for m > 16 with any c_z, and for m <= 16 with c_z == 0), an Inf in x
at a skipped position, the same bits from the same call twice, and the layer and the two network functions on a hand-built network."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from tests.helpers import grouped_ref, sparse_ref  # noqa: E402
from tests.helpers import grouped_sparse_ref as ref  # noqa: E402
from tests.helpers.cbmm_ref import relu_like_torch  # noqa: E402
from tests.helpers.grouped_sparse_ref import CASES  # noqa: E402


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import ops

    _, cus = ops.device_info()
    assert cus >= 1
    return types.SimpleNamespace(ops=ops, cus=cus)


def _dev(host, view=False):
    """host float32 values -> device tensor; ``view``: as buf[1:] of a one-longer buffer (4-byte aligned and no further)."""
    host = np.ascontiguousarray(host, dtype=np.float32)
    if not view:
        return torch.from_numpy(host).cuda()
    buf = torch.zeros(host.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(host.ravel()).cuda()
    return buf[1:].view(host.shape)


def _dev_labels(lab, off=0):
    """The indices as uint8 starting ``off`` bytes into a larger buffer."""
    host = np.ascontiguousarray(np.asarray(lab).ravel().astype(np.uint8))
    buf = torch.zeros(off + host.size + 16, dtype=torch.uint8, device="cuda")
    buf[off: off + host.size] = torch.from_numpy(host).cuda()
    return buf[off: off + host.size]


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def case_data(env):
    """Per case, made once and left unchanged: exact and float data on the host, the labels and their packed form on the device."""
    out = []
    for ci, c in enumerate(CASES):
        lab, zs, x, cen, bias = ref.exact_data(c, 100 + ci, ci)
        xf, cf, bf = ref.float_data(c, zs, 100 + ci)
        lab_t = _dev_labels(lab, c["off"])
        assert lab_t.storage_offset() == c["off"]
        zs_t = torch.from_numpy(zs).cuda()
        codes = env.ops.pack_grouped_sparse_codes(lab_t, c["kdim"], c["ncols"], c["k"], c["group_rows"], zero_symbols=zs_t)
        out.append(dict(lab=lab, zs=zs, x=x, cen=cen, bias=bias, xf=xf, cf=cf, bf=bf, lab_t=lab_t, zs_t=zs_t, codes=codes))
    return out


IDS = [ref.case_id(c) for c in CASES]


def test_the_case_list_hits_every_regime_at_this_device(env):
    seen, feats = set(), set()
    for c in CASES:
        plan = env.ops.cbsp_grouped_plan(c["m"], c["kdim"], c["ncols"], c["k"], c["group_rows"], env.cus)
        seen.add(ref.regime_of(plan))
        feats |= ref.features_of(c, plan)
    assert ref.required_regimes() <= seen, ref.required_regimes() - seen
    assert ref.required_features() <= feats, ref.required_features() - feats


# ------------------------------------------------------------------ equality 5: the pack
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_pack_is_the_numpy_buffer_and_unpack_its_inverse(env, case_data, ci):
    c, d = CASES[ci], case_data[ci]
    kdim, ncols, rows = c["kdim"], c["ncols"], c["group_rows"]
    codes = d["codes"]
    want = ref.pack_np(d["lab"], kdim, ncols, rows, d["zs"])
    assert codes.nnz == want["nnz"] == int(ref.keep_mask(d["lab"], d["zs"], rows).sum())
    L = sparse_ref.layout(kdim, ncols, 1, codes.nnz)
    assert codes.buf.numel() == L["bytes"] and codes.buf.data_ptr() % 256 == 0
    assert codes.nbytes() == L["bytes"] + len(d["zs"]) and codes.groups == len(d["zs"])
    assert abs(codes.density() - want["nnz"] / (kdim * ncols)) < 1e-12
    raw = codes.buf.cpu().numpy()
    bitmap, counts, sym = sparse_ref.split_packed(raw, kdim, ncols, 1, codes.nnz)
    assert np.array_equal(bitmap, want["bitmap"]) and np.array_equal(counts, want["counts"])
    assert np.array_equal(sym, want["symbols"].astype(np.uint8))
    back = codes.to_dense()
    assert back.dtype == torch.uint8 and np.array_equal(back.cpu().numpy().reshape(kdim, ncols), d["lab"].astype(np.uint8))


def test_default_zero_symbols_are_the_most_frequent_per_group_ties_to_the_lowest(env):
    rng = np.random.RandomState(11)
    kdim, ncols, k, rows = 100, 70, 16, 32
    lab = np.concatenate([sparse_ref.labels_at_density(rng, 32, ncols, k, 0.2, 7), sparse_ref.labels_at_density(rng, 32, ncols, k, 0.3, 0),
                          np.tile(np.array([5, 2], dtype=np.int64), (32, ncols // 2)),           # a tie of 5 and 2: the lowest
                          sparse_ref.labels_at_density(rng, 4, ncols, k, 0.1, 15)], axis=0)
    codes = env.ops.pack_grouped_sparse_codes(_dev_labels(lab, 1), kdim, ncols, k, rows)
    want = np.array([np.argmax(np.bincount(lab[g * rows: (g + 1) * rows].ravel(), minlength=k)) for g in range(4)])
    assert np.array_equal(want, [7, 0, 2, 15])
    assert codes.zero_symbols.dtype == torch.uint8 and np.array_equal(codes.zero_symbols.cpu().numpy(), want)
    assert codes.nnz == int(ref.keep_mask(lab, want, rows).sum())
    assert np.array_equal(codes.to_dense().cpu().numpy().reshape(kdim, ncols), lab)
    with pytest.raises(ValueError, match="one byte per group"):
        env.ops.pack_grouped_sparse_codes(_dev_labels(lab), kdim, ncols, k, rows, zero_symbols=torch.zeros(3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="multiple of 32"):
        env.ops.pack_grouped_sparse_codes(_dev_labels(lab), kdim, ncols, k, 48)
    with pytest.raises(TypeError, match="uint8"):
        env.ops.pack_grouped_sparse_codes(torch.zeros(kdim * ncols, dtype=torch.int16, device="cuda"), kdim, ncols, k, rows)


# ------------------------------------------------------------------ equality 1: exact data
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_exact_data_is_the_float64_formula_and_the_byte_form_bit_for_bit(env, case_data, ci):
    c, d = CASES[ci], case_data[ci]
    ops = env.ops
    want = ref.formula64(d["x"], d["lab"], d["cen"], d["zs"], c["group_rows"], d["bias"])
    x_t, cen_t = _dev(d["x"], c["x_view"]), _dev(d["cen"])
    bias_t = None if d["bias"] is None else _dev(d["bias"])
    unpacked = d["codes"].to_dense()
    with torch.no_grad():
        for relu in (False, True):
            w64 = relu_like_torch(want) if relu else want
            y = ops.grouped_sparse_codebook_matmul(x_t, d["codes"], cen_t, bias=bias_t, relu=relu)
            assert y.shape == (c["m"], c["ncols"]) and y.dtype == torch.float32
            got = y.cpu().numpy()
            assert np.array_equal(got.astype(np.float64), w64), (relu, float(np.abs(got - w64).max()))
            yb = ops.grouped_codebook_matmul(x_t, unpacked, cen_t, c["kdim"], c["ncols"], c["group_rows"], bias=bias_t, relu=relu)
            assert torch.equal(y, yb), relu
            again = ops.grouped_sparse_codebook_matmul(x_t, d["codes"], cen_t, bias=bias_t, relu=relu)
            assert torch.equal(_bits(y), _bits(again))   # determinism: the same call, the same bits


# ------------------------------------------------------------------ equality 4: float data
@pytest.mark.parametrize("ci", range(len(CASES)), ids=IDS)
def test_float_data_is_within_the_derived_bound(env, case_data, ci):
    c, d = CASES[ci], case_data[ci]
    want, bound = ref.float_bound(d["xf"], d["lab"], d["cf"], d["zs"], c["group_rows"], d["bf"])
    x_t, cen_t = _dev(d["xf"], c["x_view"]), _dev(d["cf"])
    bias_t = None if d["bf"] is None else _dev(d["bf"])
    with torch.no_grad():
        y = env.ops.grouped_sparse_codebook_matmul(x_t, d["codes"], cen_t, bias=bias_t)
        again = env.ops.grouped_sparse_codebook_matmul(x_t, d["codes"], cen_t, bias=bias_t)
    err = np.abs(y.cpu().numpy().astype(np.float64) - want)
    print(f"{ref.case_id(c)}: largest err / bound = {float((err / bound).max()):.4f}")
    assert np.all(err <= bound)
    assert torch.equal(_bits(y), _bits(again))


# ------------------------------------------------------------------ equalities 2 and 3: one group against the ungrouped sparse product
ONE_GROUP = [(17, 112, 130, 16), (17, 300, 50, 256), (130, 300, 129, 3), (300, 40, 64, 16),                           # m > 16: direct, split, two tiles
             (1, 112, 70, 16), (2, 200, 1, 3), (4, 130, 64, 256), (8, 63, 50, 16), (16, 112, 130, 16),                # m <= 16 direct
             (1, 1000, 50, 16), (2, 1500, 64, 3), (4, 1000, 130, 256), (8, 2100, 50, 16), (16, 1000, 70, 16)]         # m <= 16 split


@pytest.mark.parametrize("m,kdim,ncols,k", ONE_GROUP, ids=[f"m{a}-kd{b}-n{c}-k{d}" for a, b, c, d in ONE_GROUP])
def test_one_group_is_the_ungrouped_sparse_product(env, m, kdim, ncols, k):
    ops = env.ops
    rng = np.random.RandomState(m * 1000 + kdim)
    z = 3 % k
    lab = sparse_ref.labels_at_density(rng, kdim, ncols, k, 0.15, z)
    lab_t = _dev_labels(lab, 1)
    rows = -(-kdim // 32) * 32 + 32 * (m % 2)                      # group_rows >= kdim: kdim rounded up, and beyond
    zs_t = torch.tensor([z], dtype=torch.uint8, device="cuda")
    gcodes = ops.pack_grouped_sparse_codes(lab_t, kdim, ncols, k, rows, zero_symbols=zs_t)
    scodes = ops.pack_sparse_codes(lab_t, kdim, ncols, k, zero_symbol=z)
    assert gcodes.nnz == scodes.nnz
    L = sparse_ref.layout(kdim, ncols, 1, gcodes.nnz)
    both = [t.cpu().numpy() for t in (gcodes.buf, scodes.buf)]
    for a, b in ((0, L["off_hi"] + 4 * kdim), (L["off_sym"], L["bytes"])):   # the structure and the symbols: the same bytes
        assert np.array_equal(both[0][a:b], both[1][a:b])
    x = rng.standard_normal((m, kdim)).astype(np.float32)
    cen = rng.standard_normal(k).astype(np.float32)
    bias = rng.standard_normal(ncols).astype(np.float32)
    x_t, bias_t = _dev(x), _dev(bias)
    for cz_zero in (True, False):
        cc = cen.copy()
        if cz_zero:
            cc[z] = 0.0
        cen_t = _dev(cc)
        with torch.no_grad():
            for relu in (False, True):
                got = ops.grouped_sparse_codebook_matmul(x_t, gcodes, cen_t.view(1, k), bias=bias_t, relu=relu)
                want = ops.sparse_codebook_matmul(x_t, scodes, cen_t, bias=bias_t, relu=relu)
                if m > 16 or cz_zero:
                    assert torch.equal(got, want), (cz_zero, relu)
                elif not relu:
                    # m <= 16 and c_z != 0: the ungrouped kernel sums the row inside its stream kernel in another order, so the
                    # two agree only within the float bound; each is within it of the float64 product
                    r64, bound = ref.float_bound(x, lab, cc.reshape(1, k), np.array([z], dtype=np.uint8), rows, bias)
                    for y in (got, want):
                        assert np.all(np.abs(y.cpu().numpy().astype(np.float64) - r64) <= bound)


# ------------------------------------------------------------------ the departure, per group: an Inf in x at a skipped position
@pytest.mark.parametrize("m", [1, 17])
def test_inf_at_a_skipped_position_of_a_group_with_zero_cz_makes_no_nan(env, m):
    ops = env.ops
    rng = np.random.RandomState(5 + m)
    kdim, ncols, k, rows = 96, 70, 16, 32
    zs = np.array([3, 5, 7], dtype=np.uint8)
    lab = np.concatenate([sparse_ref.labels_at_density(rng, rows, ncols, k, 0.3, int(z)) for z in zs], axis=0)
    lab[40] = 5                                                    # row 40 (group 1) is skipped entirely
    cen = (rng.standard_normal((3, k)) + 2.0).astype(np.float32)
    cen[1, 5] = 0.0                                                # c_{z_1} == 0 exactly; the other two groups keep their rank-1 terms
    x = rng.standard_normal((m, kdim)).astype(np.float32)
    x[m - 1, 40] = np.inf
    codes = ops.pack_grouped_sparse_codes(_dev_labels(lab), kdim, ncols, k, rows, zero_symbols=torch.from_numpy(zs).cuda())
    x_t, cen_t = _dev(x), _dev(cen)
    with torch.no_grad():
        y = ops.grouped_sparse_codebook_matmul(x_t, codes, cen_t).cpu().numpy()
        yb = ops.grouped_codebook_matmul(x_t, _dev_labels(lab), cen_t, kdim, ncols, rows).cpu().numpy()
    assert np.isfinite(y).all()                                    # the skipped weights of group 1 are absent: Inf meets no 0
    assert np.isnan(yb[m - 1]).all() and np.isfinite(yb[: m - 1]).all()   # the byte form multiplies Inf by the 0 centre
    want = ref.formula64(x, lab, cen, zs, rows)
    xz = x.copy()
    xz[m - 1, 40] = 0.0
    r64, bound = ref.float_bound(xz, lab, cen, zs, rows)
    assert np.isfinite(want).all() and np.all(np.abs(y.astype(np.float64) - r64) <= bound)


@pytest.mark.parametrize("m", [1, 17])
@pytest.mark.parametrize("groups,rows", [(260, 32), (5, 320)], ids=["260x32", "5x320"])
def test_the_rowterm_pass_over_many_groups_and_over_long_groups(env, m, groups, rows):
    """k_cbspg_rowterm takes the groups in chunks of 256 (260 groups of 32 rows: t summed in group order across the chunks), and a
    wave that takes a group of more than 256 rows on its own sums it thread-strided (5 groups of 320 rows).  Exact data without the
    per-group offset (260 offsets of 64 g would pass 2^24 quarter-units): |c| <= 4, x in {-1, 0, 1}, so the magnitudes of an
    output's terms sum to less than 4 * 4 * kdim quarter-units."""
    ops = env.ops
    rng = np.random.RandomState(77 + m + groups)
    kdim, ncols, k = rows * groups, 3, 4
    zs = (np.arange(groups) % k).astype(np.uint8)
    lab = np.concatenate([sparse_ref.labels_at_density(rng, rows, ncols, k, 0.2, int(z)) for z in zs], axis=0)
    cen = (rng.randint(-16, 17, size=(groups, k)) / 4.0).astype(np.float32)
    cen[3, zs[3]] = 0.0
    x = rng.randint(-1, 2, size=(m, kdim)).astype(np.float32)
    assert 4.0 * ref._magnitude(x, lab, cen, zs, rows, None).max() < 2.0 ** 24
    codes = ops.pack_grouped_sparse_codes(_dev_labels(lab, 1), kdim, ncols, k, rows, zero_symbols=torch.from_numpy(zs).cuda())
    with torch.no_grad():
        y = ops.grouped_sparse_codebook_matmul(_dev(x), codes, _dev(cen)).cpu().numpy()
    assert np.array_equal(y.astype(np.float64), ref.formula64(x, lab, cen, zs, rows))


# ------------------------------------------------------------------ the op's rules
def test_the_op_refuses_half_inputs_autograd_and_wrong_shapes(env, case_data):
    ops = env.ops
    c, d = CASES[0], case_data[0]
    x_t, cen_t = _dev(d["x"]), _dev(d["cen"])
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="float32 activations"):
            ops.grouped_sparse_codebook_matmul(x_t.to(dt), d["codes"], cen_t)
    xg = x_t.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="inference only"):
        ops.grouped_sparse_codebook_matmul(xg, d["codes"], cen_t)
    with pytest.raises(TypeError, match="GroupedSparseCodes"):
        ops.grouped_sparse_codebook_matmul(x_t, d["lab_t"], cen_t)
    with pytest.raises(ValueError, match="centers must have shape"):
        ops.grouped_sparse_codebook_matmul(x_t, d["codes"], cen_t[:1])
    with pytest.raises(ValueError, match="x must have shape"):
        ops.grouped_sparse_codebook_matmul(x_t[:, :-1].contiguous(), d["codes"], cen_t)
    with torch.no_grad():
        y3 = ops.grouped_sparse_codebook_matmul(x_t.view(1, c["m"], c["kdim"]), d["codes"], cen_t)      # leading dimensions are kept
        assert y3.shape == (1, c["m"], c["ncols"])
        assert ops.grouped_sparse_codebook_matmul(x_t[:0], d["codes"], cen_t).shape == (0, c["ncols"])  # m = 0: a no-op
    # kdim = 0 writes the bias
    empty = ops.pack_grouped_sparse_codes(torch.zeros(0, dtype=torch.uint8, device="cuda"), 0, 5, 4, 32)
    assert empty.nnz == 0 and empty.groups == 0
    bias = torch.arange(5, dtype=torch.float32, device="cuda") - 2
    with torch.no_grad():
        y0 = ops.grouped_sparse_codebook_matmul(torch.zeros(3, 0, device="cuda"), empty, torch.zeros(1, 4, device="cuda"), bias=bias, relu=True)
    assert torch.equal(y0, torch.relu(bias).expand(3, 5))


# ------------------------------------------------------------------ the layer and the network functions
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


def _grouped_layer(compressed, rng, kdim, ncols, k, rows, density, activation, exact):
    c = dict(kdim=kdim, ncols=ncols, k=k, group_rows=rows)
    zs = (1 + 2 * np.arange(ref.groups_of(c))) % k
    lab = np.concatenate([sparse_ref.labels_at_density(rng, min(kdim, (g + 1) * rows) - g * rows, ncols, k, density, int(z))
                          for g, z in enumerate(zs)], axis=0)
    if exact:
        cen = (rng.randint(-8, 9, size=(len(zs), k)) / 4.0).astype(np.float32)
        bias = rng.randint(-5, 6, size=ncols).astype(np.float32)
    else:
        cen = (rng.standard_normal((len(zs), k)) * 0.2).astype(np.float32)
        bias = rng.standard_normal(ncols).astype(np.float32)
    return compressed.GroupedCompressedDense.from_codes(kdim, ncols, rows, _dev_labels(lab, 1), _dev(cen), _dev(bias), activation), lab, zs


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "float"])
def test_the_layer_and_sparsify_grouped_layers(env, exact):
    from neural_network_compression_amd import compressed

    rng = np.random.RandomState(21)
    l1, lab1, zs1 = _grouped_layer(compressed, rng, 96, 64, 16, 32, 0.1, torch.relu, exact)
    l2, lab2, zs2 = _grouped_layer(compressed, rng, 64, 10, 16, 32, 0.1, None, exact)
    net = _Net(fc1=l1, fc2=l2)
    full = compressed.sparsify_grouped_layers(net)                       # sparse=True: both layers
    assert type(full.fc1) is type(full.fc2) is compressed.GroupedSparseCompressedDense
    assert type(net.fc1) is type(net.fc2) is compressed.GroupedCompressedDense   # a deep copy: net is as it was
    auto = compressed.sparsify_grouped_layers(net, sparse="auto")
    assert type(auto.fc1) is compressed.GroupedSparseCompressedDense and type(auto.fc2) is compressed.GroupedCompressedDense   # 16 B of structure per 10-column row

    s1, s2 = full.fc1, full.fc2
    assert np.array_equal(s1.zero_symbols.cpu().numpy(), zs1) and np.array_equal(s2.zero_symbols.cpu().numpy(), zs2)   # the pruned cluster is the most frequent
    for s, b, lab, zs in ((s1, l1, lab1, zs1), (s2, l2, lab2, zs2)):
        nnz = int(ref.keep_mask(lab, zs, 32).sum())
        parts = sparse_ref.layout(b.kdim, b.ncols, 1, nnz)["bytes"] + len(zs) + 4 * len(zs) * 16 + 4 * b.ncols
        assert s.nnz == nnz and s.nbytes() == parts == compressed.compressed_nbytes(s)
        assert s.get_weights() == [] and torch.equal(s.codes.to_dense(), b.labels)
    assert compressed.compressed_nbytes(full) == s1.nbytes() + s2.nbytes()
    assert s2.nbytes() > l2.nbytes() and s1.nbytes() < l1.nbytes()
    assert compressed.compressed_nbytes(auto) == s1.nbytes() + l2.nbytes() < compressed.compressed_nbytes(full) < compressed.compressed_nbytes(net)

    m = 5
    x = rng.randint(-4, 5, size=(m, 96)).astype(np.float32) if exact else rng.standard_normal((m, 96)).astype(np.float32)
    xt = _dev(x)
    with torch.no_grad():
        h = xt
        for name in ("fc1", "fc2"):
            a, b = getattr(net, name), getattr(full, name)
            ya, yb = a(h), b(h)
            if exact:
                assert torch.equal(ya, yb), name
            else:
                lab, zs = (lab1, zs1) if name == "fc1" else (lab2, zs2)
                hn = h.cpu().numpy()
                r64, bound = ref.float_bound(hn, lab, a.centers.cpu().numpy(), zs, 32, a.bias.cpu().numpy())
                r64 = relu_like_torch(r64) if a.activation is torch.relu else r64
                assert np.all(np.abs(yb.cpu().numpy().astype(np.float64) - r64) <= bound), name
                # the byte form is within section 17's bound of the same product, so the two layers are within the sum of both
                w = grouped_ref.weights(a.centers.cpu().numpy(), lab, a.kdim, a.ncols, 32).astype(np.float64)
                byte_bound = 2 * a.kdim * ref.U * (np.abs(hn.astype(np.float64)) @ np.abs(w) + np.abs(a.bias.cpu().numpy().astype(np.float64)))
                assert np.all(np.abs(yb.cpu().numpy().astype(np.float64) - ya.cpu().numpy().astype(np.float64)) <= bound + byte_bound), name
            h = ya
        assert torch.equal(_bits(full(xt)), _bits(full(xt)))
        if exact:
            assert torch.equal(full(xt), net(xt)) and torch.equal(auto(xt), net(xt))
        y_nc = full.fc1(_dev(np.ascontiguousarray(x.T)).t())              # a non-contiguous view of the same values
        assert torch.equal(_bits(y_nc), _bits(full.fc1(xt)))
    with pytest.raises(TypeError, match="float32 activations"):
        full.fc1(xt.to(torch.bfloat16))
    with pytest.raises(RuntimeError, match="inference only"):
        full.fc1(xt.clone().requires_grad_(True))
    for bad in (False, None, "yes", 1.5, 1):
        with pytest.raises(ValueError, match="sparse"):
            compressed.sparsify_grouped_layers(net, sparse=bad)

    # packed grouped layers and all other layers are left alone
    mixed = _Net(fc1=compressed.GroupedPackedCompressedDense.from_grouped(l1), fc2=l2)
    out = compressed.sparsify_grouped_layers(mixed)
    assert type(out.fc1) is compressed.GroupedPackedCompressedDense and type(out.fc2) is compressed.GroupedSparseCompressedDense

    # the state dict round trip keeps the layer
    clone = compressed.GroupedSparseCompressedDense.from_grouped(l1)
    clone.load_state_dict(s1.state_dict())
    with torch.no_grad():
        assert torch.equal(_bits(clone(xt)), _bits(s1(xt)))


def test_smallest_grouped_layers_picks_by_bytes(env):
    from neural_network_compression_amd import compressed

    rng = np.random.RandomState(33)
    pruned, _, _ = _grouped_layer(compressed, rng, 96, 64, 16, 32, 0.1, torch.relu, True)     # sparse < packed < byte
    dense, _, _ = _grouped_layer(compressed, rng, 64, 64, 16, 32, 1.0, torch.relu, True)      # packed < byte < sparse
    tie, _, _ = _grouped_layer(compressed, rng, 64, 16, 16, 32, 1.0, torch.relu, True)        # 16-byte packed rows of 16 columns: byte == packed
    wide, _, _ = _grouped_layer(compressed, rng, 16, 10, 17, 32, 1.0, None, True)             # K = 17: no packed form; 10 columns: byte
    wide_pruned, _, _ = _grouped_layer(compressed, rng, 96, 64, 17, 32, 0.1, None, True)      # K = 17 and pruned: sparse
    net = _Net(a=pruned, b=dense, c=tie, d=wide)
    out = compressed.smallest_grouped_layers(net)
    for name, layer in net.get_config().items():
        cands = [layer]
        if layer.centers.shape[1] <= 16:
            cands.append(compressed.GroupedPackedCompressedDense.from_grouped(layer))
        cands.append(compressed.GroupedSparseCompressedDense.from_grouped(layer))
        best = min(cands, key=lambda l: l.nbytes())          # min keeps the first of equals: byte, then packed, then sparse
        assert type(getattr(out, name)) is type(best) and getattr(out, name).nbytes() == best.nbytes(), name
    assert type(out.a) is compressed.GroupedSparseCompressedDense and type(out.b) is compressed.GroupedPackedCompressedDense
    assert tie.nbytes() == compressed.GroupedPackedCompressedDense.from_grouped(tie).nbytes() and type(out.c) is compressed.GroupedCompressedDense
    assert type(out.d) is compressed.GroupedCompressedDense and type(net.a) is compressed.GroupedCompressedDense
    assert type(compressed.smallest_grouped_layers(_Net(a=wide_pruned)).a) is compressed.GroupedSparseCompressedDense
    x = _dev(rng.randint(-3, 4, size=(4, 96)).astype(np.float32))
    with torch.no_grad():
        assert torch.equal(out.a(x), net.a(x))
    assert compressed.compressed_nbytes(out) == sum(layer.nbytes() for layer in out.get_config().values()) < compressed.compressed_nbytes(net)


def test_the_old_doors_still_refuse_grouped_layers(env):
    """compress_network(..., sparse=...) names a layer with group-wise codebooks and raises, before anything is built; the way to the
    bitmap-sparse grouped form is sparsify_grouped_layers on the result."""
    from neural_network_compression_amd import compressed

    rng = np.random.RandomState(4)
    layer, _, _ = _grouped_layer(compressed, rng, 64, 10, 16, 32, 0.1, None, True)
    net = _Net(fc1=layer)
    models = {layer: [types.SimpleNamespace(group_rows=32), None]}
    for option in (True, "auto"):
        with pytest.raises(NotImplementedError, match="fc1"):
            compressed.compress_network(net, models, sparse=option)
