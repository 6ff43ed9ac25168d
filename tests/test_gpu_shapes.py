"""The device half of the chain on heavy-tailed, offset and few-valued weights (run with -m gpu on an MI355X).

Every other tensor the suite feeds to the device is a zero-mean bell (synth.weights).  The code that is hardest to get right depends
on the DATA: the uniform cell grid of the E-step (a few outliers put the whole bulk into one cell), the width of the sort keys (the
bounded form or the fall-back), the 31-bin histogram behind the density init (mass in one bin: duplicate initial centres, mass
empty-cluster events, ties at the selection cut), the fixed-point shift (set by the largest |x - mean|), centring data whose mean
is 50 sigma away, a prune threshold set by a few values.  The inputs are the recipes of tests/helpers/shapes.py; the goldens
(tests/golden/ref_shapes.*) are what the reference itself produced on them, and the CPU oracle is pinned to those bit for bit by
tests/test_oracle_shapes.py.  Here the device is held to the oracle in the device's arithmetic bit for bit, to the CPU-computed gap
to the reference exactly, and -- in the reference's own arithmetic -- to the reference bit for bit.  No tolerance of its own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import oracle as orc  # noqa: E402
from tests.helpers import ab_gap, shapes  # noqa: E402

G = shapes.goldens()
bits = shapes.f32_bits


@pytest.fixture(scope="module")
def nnc():
    assert torch.cuda.is_available(), "these tests need the GPU"
    from neural_network_compression_amd import _native, compressed, kmeans, ops, pipeline, storage
    from neural_network_compression_amd.common import utility

    class NS:
        pass

    ns = NS()
    ns.L = _native.load()   # fails loudly if the HIP library is missing
    ns.nat, ns.ops, ns.kmeans, ns.utility, ns.pipeline, ns.storage, ns.compressed = _native, ops, kmeans, utility, pipeline, storage, compressed
    return ns


def dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).cuda()     # (the cached inputs are read-only)


def host_labels(lab):
    return (lab.to(torch.int32).cpu().numpy() & 0xFFFF).astype(np.int32)


# ------------------------------------------------------------------ a. statistics and prune, against NumPy itself
@pytest.mark.parametrize("n", [3000, 8193, 50_000])
@pytest.mark.parametrize("name", shapes.SHAPES)
def test_statistics_and_prune_equal_numpy(nnc, name, n):
    w = shapes.make(name, n)
    x = dev(w)
    mean, var, std = nnc.ops.moments(x)
    assert bits(mean.item()) == bits(np.mean(w)) and bits(var.item()) == bits(np.var(w)) and bits(std.item()) == bits(np.std(w))

    def check_stats(st, mm, signs, v):
        nzv = v[v != 0]
        want = [v.min(), v.max(), nzv.min() if nzv.size else np.float32(np.inf), nzv.max() if nzv.size else np.float32(-np.inf)]
        if st is not None:
            assert bits(st.mean) == bits(np.mean(v)) and bits(st.var) == bits(np.var(v))
            assert [bits(t) for t in (st.min, st.max, st.min_nonzero, st.max_nonzero)] == [bits(t) for t in want]
            assert (st.n_negative, st.n_zero) == (int((v < 0).sum()), int((v == 0).sum()))
        if mm is not None:
            assert [bits(t) for t in mm.cpu().numpy()] == [bits(t) for t in want]
            assert [int(t) for t in signs.cpu().numpy()] == [int((v < 0).sum()), int((v == 0).sum())]

    check_stats(nnc.kmeans.LayerStats(x), *nnc.ops.minmax_signs(x), w)
    q = 1.0
    sigma = np.std(w)
    thr = sigma * q                                   # float32, as the reference computes it (utility.py:159)
    want_mask = np.abs(w) < thr
    pruned = w.copy()
    pruned[want_mask] = 0
    a, b = dev(w), dev(w)
    m1, s1, z1 = nnc.ops.prune_(a, q, True)
    m2, s2, z2, mm2, sg2 = nnc.ops.prune_stats_(b, q, True)
    for m, s, z, t in ((m1, s1, z1, a), (m2, s2, z2, b)):
        assert np.array_equal(m.cpu().numpy().astype(bool), want_mask)
        assert [bits(v) for v in s.cpu().numpy()] == [bits(sigma), bits(thr)]
        assert int(z.item()) == int(want_mask.sum())
        assert np.array_equal(t.cpu().numpy().view(np.uint32), pruned.view(np.uint32))
    check_stats(nnc.kmeans.LayerStats(a), mm2, sg2, pruned)
    ikey = shapes.input_key(name, n, q)
    if ikey in G.inputs:                               # ... and the reference's own mask
        i = G.inputs[ikey]
        assert shapes.sha(w) == i["input_sha256"] and bits(sigma) == i["sigma_bits"]
        assert shapes.sha(np.packbits(m1.cpu().numpy().astype(bool))) == i["mask_sha256"] and int(z1.item()) == i["nzeroed"]
        mask_u = nnc.utility.prune_weigth(w.copy(), threshold=q, std_smooth=True)
        assert shapes.sha(np.packbits(mask_u.ravel())) == i["mask_sha256"]


# ------------------------------------------------------------------ b. both forms of the sort of a pruned vector
SORT_QS = (1.0, 0.05)      # the goldens' threshold; and one that keeps the bulk, so that the surviving range is the input's own
_SORT_BITS: dict = {}


def _sort_forms(nnc, name, n, q):
    """Key width nnc_sort_pruned_bounded_bits gives the pruned tensor (0: the bounded form does not apply), after checking every
    form of the sort that applies against np.sort."""
    if (name, n, q) in _SORT_BITS:
        return _SORT_BITS[(name, n, q)]
    L, ops = nnc.L, nnc.ops
    x = dev(shapes.make(name, n))
    mask, stats, nz, mm, signs = ops.prune_stats_(x, q, True)
    thr = float(stats.cpu().numpy()[1])
    mmh, sg = mm.cpu().numpy(), signs.cpu().numpy()
    n_neg, n_zero = int(sg[0]), int(sg[1])
    want = np.sort(x.cpu().numpy())
    stream = torch.cuda.current_stream().cuda_stream
    kb = int(L.nnc_sort_pruned_bounded_bits(float(mmh[0]), float(mmh[1]), thr, n_neg, n - n_neg - n_zero))
    assert 0 <= kb <= 27
    if kb > 0:
        out = torch.empty_like(x)
        wsb = int(L.nnc_sort_pruned_bounded_workspace_bytes(n - n_zero))
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        nnc.nat.check(L.nnc_sort_pruned_bounded_f32(x.data_ptr(), n, n_neg, n_zero, float(mmh[0]), float(mmh[1]), thr, out.data_ptr(), ws.data_ptr(), wsb, stream))
        assert np.array_equal(out.cpu().numpy(), want), (name, n, q, "bounded")
        off = L.nnc_sort_pruned_bounded_flag(ws.data_ptr(), n - n_zero) - ws.data_ptr()
        assert int(ws[off: off + 4].view(torch.int32).item()) == 0          # every weight inside the bounds it was given
    out = torch.empty_like(x)                                               # the fall-back (and what a fit outside the layer call takes)
    wsb = int(L.nnc_sort_pruned_workspace_bytes(n, n_neg, n_zero))
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    nnc.nat.check(L.nnc_sort_pruned_f32(x.data_ptr(), n, n_neg, n_zero, out.data_ptr(), ws.data_ptr(), wsb, stream))
    assert np.array_equal(out.cpu().numpy(), want), (name, n, q, "pruned")
    st = nnc.kmeans.LayerStats(x)
    assert (st.n_negative, st.n_zero) == (n_neg, n_zero)
    assert np.array_equal(nnc.kmeans.sorted_copy(x, st).cpu().numpy(), want), (name, n, q, "sorted_copy")
    _SORT_BITS[(name, n, q)] = kb
    return kb


@pytest.mark.parametrize("name", shapes.SHAPES)
def test_sorted_copy_of_the_pruned_tensor_in_every_form(nnc, name):
    for n in (6000, 50_000):
        for q in SORT_QS:
            kb = _sort_forms(nnc, name, n, q)
            print(f"sort {name} n={n} q={q}: {'bounded, ' + str(kb) + ' key bits' if kb else 'fall-back (more than 27 key bits)'}")


def test_both_sort_forms_are_taken(nnc):
    kb = {(name, q): _sort_forms(nnc, name, 50_000, q) for name in shapes.SHAPES for q in SORT_QS}
    # a few extreme values stretch the surviving range past 27 key bits once the bulk survives the threshold: the general sort takes over
    assert kb[("outliers", 0.05)] == 0 and kb[("quintic", 0.05)] == 0 and kb[("cubic", 0.05)] == 0
    assert sum(1 for v in kb.values() if v > 0) >= 8 and kb[("onesided", 1.0)] > 0 and kb[("gain", 1.0)] > 0


# ------------------------------------------------------------------ c. weight distribution and initial centres
def _u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _u32(a):
    a = np.asarray(a)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("ikey", sorted(G.inputs))
def test_weight_distribution_and_init_equal_the_reference(nnc, ikey):
    i = G.inputs[ikey]
    w = shapes.pruned_input(i["shape"], i["n"], i["q"])[0]
    gx, gc = G.cdfs(i)
    x = dev(w)
    st = nnc.kmeans.LayerStats(x)
    results = {
        "host": nnc.utility.get_weight_distribution(w[w != 0]),
        "device": nnc.utility.get_weight_distribution(dev(w[w != 0])),
        "skip_zeros": nnc.utility.get_weight_distribution(x, skip_zeros=True),
        "sorted": nnc.pipeline.weight_distribution_sorted(nnc.kmeans.sorted_copy(x, st), st),
    }
    for how, (xnew, cdf) in results.items():
        assert np.array_equal(_u32(xnew), _u32(gx)), (ikey, how)
        assert np.array_equal(_u64(cdf), _u64(gc)), (ikey, how)
    checked = 0
    for key in G.fits():
        c = G.cases[key]
        if shapes.input_key(c["shape"], c["n"], c["q"]) != ikey:
            continue
        if c["forgy_seed"] is not None:
            np.random.seed(c["forgy_seed"])
        space = np.asarray(nnc.utility._init_space(x, x.numel(), c["bits"], c["mode"], results["sorted"] if c["mode"] == "density" else None), dtype=np.float32)
        assert np.array_equal(_u32(space), _u32(G.init(c))), key
        if c["mode"] != "forgy":
            assert np.array_equal(_u32(nnc.pipeline.initial_centroids(x, c["bits"], c["mode"], results["skip_zeros"])), _u32(G.init(c))), key
        checked += 1
    assert checked >= 1


# ------------------------------------------------------------------ oracle fits, shared
_ORC: dict = {}


def oracle_fit(key, accum):
    """The oracle's fit of a golden case from the golden's own initial centres: accum = "device" (what device_arith says for the size:
    mode B, or the reference's sums with the device's relocation rule up to 4096 weights) or "B".  Computed once."""
    c = G.cases[key]
    if accum == "device" and orc.device_arith(c["n"], c["K"])[0] == "B":
        accum = "B"
    if (key, accum) not in _ORC:
        kw = {} if c["max_iter"] is None else {"max_iter": c["max_iter"]}
        _ORC[(key, accum)] = orc.kmeans_lloyd(shapes.case_input(c), G.init(c), accum=accum, **kw)
    return _ORC[(key, accum)]


# ------------------------------------------------------------------ d. the E-step on every cell grid
ESTEP_SHAPES = ("outliers", "quintic", "gain", "ternary")
_ESTEP_SETS: dict = {}


def _estep_centre_sets(name, k):
    """Two sets of k centres for the unpruned 50 000-weight tensor: the reference's initial centres (k = 16: linear at 4 bits, the
    golden's; k = 65 / 257: density at 6 / 8 bits from the golden weight distribution) and where the oracle's fit has taken them (its
    final centres for k = 16, after six iterations beyond)."""
    if (name, k) not in _ESTEP_SETS:
        w = shapes.pruned_input(name, 50_000, None)[0]
        if k == 16:
            key = shapes.fit_key(name, 50_000, None, "linear", 4)
            init, moved = G.init(G.cases[key]), oracle_fit(key, "B").cluster_centers_.ravel()
        else:
            nbits = {65: 6, 257: 8}[k]
            init = np.asarray(orc.init_space(w, nbits, "density", G.cdfs(G.inputs[shapes.input_key(name, 50_000, None)])), dtype=np.float32)
            moved = orc.kmeans_lloyd(w, init, accum="B", max_iter=6).cluster_centers_.ravel()
        mean = orc.np_mean(w)
        xc = (w - mean).astype(np.float32)
        sets = []
        for cen in (init, moved):
            cen = np.ascontiguousarray(cen, dtype=np.float32)
            assert cen.size == k
            sets.append((cen, orc.estep(xc, (cen - mean).astype(np.float32))))
        _ESTEP_SETS[(name, k)] = (mean, sets)
    return _ESTEP_SETS[(name, k)]


@pytest.mark.parametrize("k", [16, 65, 257])
@pytest.mark.parametrize("name", ESTEP_SHAPES)
def test_estep_on_every_cell_grid(nnc, name, k):
    w = shapes.pruned_input(name, 50_000, None)[0]
    mean, sets = _estep_centre_sets(name, k)
    x = dev(w)
    for which, (cen, want) in enumerate(sets):
        for grid_log2 in (0, 6, 11, 14):
            km = nnc.kmeans.DeviceKMeans(x, cen, grid_log2=grid_log2)
            assert bits(km.x_mean) == bits(mean)
            lab, vals, d = km.assign(which=0, labels=True, values=True, distances=True)
            labels = host_labels(lab)
            assert np.array_equal(labels, want), (name, k, which, grid_log2, int((labels != want).sum()))
            cc = (cen - mean).astype(np.float32)
            assert np.array_equal(vals.cpu().numpy(), (cc + mean).astype(np.float32)[want]), (name, k, which, grid_log2)
            t = ((w - mean).astype(np.float32) - cc[want]).astype(np.float32)
            assert np.array_equal(d.cpu().numpy(), (t * t).astype(np.float32)), (name, k, which, grid_log2)


# ------------------------------------------------------------------ e. the fit, every form, against the oracle bit for bit
_FITS: dict = {}


def _summary(o):
    """(events, events with several empty clusters, events with a tie between two DIFFERENT values at the cut, events with any tie)
    as the oracle counted them."""
    i = o.reloc_info_
    return tuple(int(i.get(f, 0)) for f in ("reloc_events", "reloc_multi", "reloc_ties_distinct", "reloc_ties"))


def _check_tie_report(model, ob, where):
    """reloc_tie_ is set exactly where the oracle counted a tie that can matter: two different VALUES equally far at a selection cut
    (include/nnc.h, nnc_kmeans_status.reloc_ties).  The oracle's older count, reloc_ties, also takes two equal values either side of
    the cut for a tie -- the zeros of a pruned tensor, the three values of `ternary`: 44 of the 45 golden fits it counts a tie on
    have only such ties, and the device reports 0 there (measured; whichever of two equal samples goes, the sums are the same) --
    so it bounds the device's count from above and is not what the report is held to."""
    _, _, distinct, any_tie = _summary(ob)
    assert (model.reloc_tie_ != 0) == (distinct != 0), (where, model.reloc_tie_, distinct, any_tie)
    assert model.reloc_tie_ <= any_tie, (where, model.reloc_tie_, any_tie)


def _check_against_oracle(tag, key, model, vals, ob):
    c = G.cases[key]
    assert model.n_iter_ == ob.n_iter_, (tag, key, model.n_iter_, ob.n_iter_)
    assert np.array_equal(_u32(model.cluster_centers_.ravel()), _u32(ob.cluster_centers_.ravel())), (tag, key)
    lab = model.labels_
    assert np.array_equal(lab, ob.labels_), (tag, key, int((lab != ob.labels_).sum()))
    assert np.array_equal(_u32(vals.cpu().numpy()), _u32(ob.cluster_centers_.ravel()[ob.labels_])), (tag, key)
    assert np.array_equal(model.counts_device_.cpu().numpy(), np.bincount(ob.labels_, minlength=c["K"])), (tag, key)
    events, multi, distinct, any_tie = _summary(ob)
    print(f"{key} [{tag}]: n_iter {model.n_iter_}; events {model.n_relocations_}/{events}, multi {model.n_reloc_multi_}/{multi}, "
          f"tie {model.reloc_tie_}/{distinct} of {any_tie} (device/oracle)")
    assert model.n_relocations_ == events, (tag, key, model.n_relocations_, events)
    assert model.n_reloc_multi_ == multi, (tag, key, model.n_reloc_multi_, multi)
    _check_tie_report(model, ob, (tag, key))
    if c["max_iter"] is not None:
        assert model.stop_reason_ == "max_iter" and model.n_iter_ == c["max_iter"], (tag, key, model.stop_reason_)


def fit_forms(nnc, key):
    """Every form of the fit of one golden case from the golden's initial centres, each checked against the oracle bit for bit.
    Returns (and keeps) what the later tests need: the default fit's result and where each form settled its empty-cluster events."""
    if key in _FITS:
        return _FITS[key]
    c = G.cases[key]
    x = dev(shapes.case_input(c))
    init = G.init(c)
    kw = {} if c["max_iter"] is None else {"max_iter": c["max_iter"]}
    ob = oracle_fit(key, "B")
    out = {"paths": {}}
    forms = [("default", {}), ("loop", {"loop": True}), ("two_launch", {"two_launch": True})]
    if c["K"] > 64:
        forms.append(("mass_in_place", {"mass_in_place": True}))
    for tag, opt in forms:
        km = nnc.kmeans.DeviceKMeans(x, init, **opt, **kw)
        model, vals = km.fit()
        _check_against_oracle(tag, key, model, vals, ob)
        st = km.status()
        ls = km.loop_stats()
        in_place = int(st.n_in_place)
        out["paths"][tag] = {"resident_loop": bool(km.lloyd), "in_place": in_place, "windowed_chain": int(km.n_reloc_windowed) - in_place,
                             "full_chain": int(km.n_reloc_full), "loop_iterations": int(ls["loop_iterations"]),
                             "wide_iterations": int(ls["wide_iterations"]), "relocated_in_loop": int(ls["relocated_in_loop"])}
        if tag == "default":
            out["model"] = model
    print(f"{key} paths: {out['paths']}")
    if orc.device_arith(c["n"], c["K"])[0] == "A":
        # what get_quantized_weight / compress_layer run on a tensor of up to 4096 weights: one launch, the reference's own sums
        od = oracle_fit(key, "device")
        model, vals = nnc.kmeans.fit_vector(x, init, **kw)
        assert model.arith_ == "reference"
        _check_against_oracle("one_launch_reference_arithmetic", key, model, vals, od)
        out["model"] = model
    m = out.pop("model")
    out.update(n_iter=m.n_iter_, centers=m.cluster_centers_.ravel().copy(), labels_sha=shapes.sha(m.labels_.astype(np.int32)),
               bincount=np.bincount(m.labels_, minlength=c["K"]).astype(np.int64), reloc_tie=m.reloc_tie_, multi=m.n_reloc_multi_, arith=m.arith_)
    _FITS[key] = out
    return out


@pytest.mark.parametrize("key", G.fits())
def test_fit_in_every_form_equals_the_oracle(nnc, key):
    fit_forms(nnc, key)


def test_every_relocation_path_was_taken(nnc):
    """Across the golden fits, empty-cluster events were settled inside the resident loop, by the finalize step of the
    launch-per-iteration form, by the windowed relocation chain and by the full-pass chain: no path goes untested silently."""
    tot = {"in_loop": 0, "by_finalize": 0, "windowed_chain": 0, "full_chain": 0, "loop_iterations": 0, "wide_iterations": 0, "relocated_in_loop": 0}
    for key in G.fits():
        for tag, p in fit_forms(nnc, key)["paths"].items():
            tot["in_loop" if p["resident_loop"] else "by_finalize"] += p["in_place"]
            for f in ("windowed_chain", "full_chain", "loop_iterations", "wide_iterations", "relocated_in_loop"):
                tot[f] += p[f]
    print("relocation events by where they were settled, all forms of all golden fits:", tot)
    assert tot["in_loop"] > 0 and tot["by_finalize"] > 0 and tot["windowed_chain"] > 0 and tot["full_chain"] > 0, tot
    assert tot["loop_iterations"] > 0 and tot["relocated_in_loop"] > 0, tot


# ------------------------------------------------------------------ f. against what the reference produced
@pytest.mark.parametrize("key", G.fits())
def test_fit_lands_on_the_cpu_computed_gap_to_the_reference(nnc, key):
    """The device's default fit against the reference's golden: exactly the gap the oracle in the device's arithmetic has (stored
    with the case, computed on the CPU); within the project's ceilings wherever the case is not listed as divergent."""
    c, g = G.cases[key], G.cases[key]["gap"]
    f = fit_forms(nnc, key)
    err = ab_gap.centre_err(f["centers"], G.centers(c))
    l1 = int(np.abs(f["bincount"] - G.bincount(c)).sum())
    print(f"{key}: {shapes.category(c)}; n_iter {f['n_iter']} (reference {c['n_iter']}), err {err:.3e} (gap {g['err']:.3e}), hist_l1 {l1} (gap {g['hist_l1']})")
    assert f["n_iter"] == g["n_iter"] and err == g["err"] and l1 == g["hist_l1"], (key, f["n_iter"], g["n_iter"], err, g["err"], l1, g["hist_l1"])
    cat = shapes.category(c)
    if c["shape"] != "ternary":
        assert (cat == "divergent") == (key in shapes.DIVERGENT), key
    if cat != "divergent":
        assert f["n_iter"] == c["n_iter"] and err <= ab_gap.SUMMATION_ERROR_CEILING, (key, err)
        if cat == "tight":
            assert err <= ab_gap.NORTH_STAR_TOL and l1 == 0, (key, err, l1)
    if c["n"] <= 4096 and not f["multi"]:
        assert f["arith"] == "reference"
        assert np.array_equal(_u32(f["centers"]), _u32(G.centers(c))) and f["labels_sha"] == c["labels_sha256"], key


# ------------------------------------------------------------------ g. the reference's own arithmetic
@pytest.mark.parametrize("key", G.fits())
def test_reference_arithmetic_is_the_reference_bit_for_bit(nnc, key):
    """arith="reference" (scikit-learn's float32 running sums in sample order), with reloc="reference" (numpy.argpartition's own
    choice) where the oracle saw a tie at a selection cut: n_iter_, every centre and every index are the reference's."""
    c = G.cases[key]
    x = dev(shapes.case_input(c))
    kw = {} if c["max_iter"] is None else {"max_iter": c["max_iter"]}
    if c["reloc_A"].get("reloc_ties", 0):
        kw["reloc"] = "reference"
    model, vals = nnc.kmeans.fit_vector(x, G.init(c), arith="reference", **kw)
    assert model.arith_ == "reference"
    one_launch = nnc.kmeans.reference_fit_applies(c["n"], c["K"]) and "reloc" not in kw
    short_pairing = one_launch and model.n_reloc_multi_ > 0      # (the one-launch form pairs several empty clusters by its own rule)
    if not short_pairing:
        assert model.n_iter_ == c["n_iter"], (key, model.n_iter_, c["n_iter"])
        assert np.array_equal(_u32(model.cluster_centers_.ravel()), _u32(G.centers(c))), key
        assert shapes.sha(model.labels_.astype(np.int32)) == c["labels_sha256"], key
        assert np.array_equal(np.bincount(model.labels_, minlength=c["K"]), G.bincount(c)), key
    assert np.array_equal(vals.cpu().numpy(), model.cluster_centers_.ravel()[model.labels_]), key


# ------------------------------------------------------------------ h. the layer as one call
LAYER_CASES = [(name, n, 1.0, mode) for name in shapes.SHAPES for n in (6000, 50_000) for mode in ("density", "linear")]
LAYER_CASES += [(name, 50_000, 0.05, mode) for name in ("outliers", "quintic") for mode in ("density", "linear")]   # the sort's fall-back inside the layer call
LAYER_CASES += [(*shapes.FEWER_NONZERO_THAN_CENTRES[:2], 1.0, mode) for mode in ("density", "linear")]
_LAYER_ORACLE: dict = {}


def _layer_oracle(name, n, q, mode):
    """prune -> weight distribution -> initial centres -> fit in the device's arithmetic -> index histogram -> Huffman lengths, on the CPU."""
    if (name, n, q, mode) not in _LAYER_ORACLE:
        w = shapes.make(name, n)
        sigma = orc.np_std(w)
        mask = orc.prune_weigth(w, q, True)
        key = shapes.fit_key(name, n, q, mode, 4)
        if key in G.cases:
            init, ob = G.init(G.cases[key]), oracle_fit(key, "device")
            cdfs = orc.get_weight_distribution(w[w != 0]) if mode == "density" else None
            assert np.array_equal(_u32(np.asarray(orc.init_space(w, 4, mode, cdfs), dtype=np.float32)), _u32(init))
        else:
            cdfs = orc.get_weight_distribution(w[w != 0]) if mode == "density" else None
            init = np.asarray(orc.init_space(w, 4, mode, cdfs), dtype=np.float32)
            ob = orc.kmeans_lloyd(w, init, accum="device")
        counts = np.bincount(ob.labels_, minlength=init.size)
        _LAYER_ORACLE[(name, n, q, mode)] = (w, mask, sigma, ob, counts, orc.huffman_lengths(counts))
    return _LAYER_ORACLE[(name, n, q, mode)]


@pytest.mark.parametrize("name,n,q,mode", LAYER_CASES)
def test_layer_as_one_call_equals_the_oracles_pipeline(nnc, name, n, q, mode):
    """compress_layer, as one call into the library and step by step, each against the oracle's own pipeline.  The nearly-all-pruned
    tensor and the one with fewer non-zero weights than centres are among the cases: the reference fits both without an exception
    (it only warns that fewer distinct clusters than centres were found), and so must the device."""
    wp, mask, sigma, ob, counts, (lengths, lhist, total) = _layer_oracle(name, n, q, mode)
    for native in (True, False):
        x = dev(shapes.make(name, n))
        r = nnc.pipeline.compress_layer(x, q=q, bits=4, mode=mode, native=native)
        tag = (name, n, q, mode, native)
        assert np.array_equal(r.mask.cpu().numpy().astype(bool).ravel(), mask) and r.nzeroed == int(mask.sum()), tag
        assert bits(r.sigma) == bits(sigma) and bits(r.threshold) == bits(orc.prune_threshold_f32(sigma, q, True)), tag
        assert np.array_equal(_u32(x.cpu().numpy()), _u32(wp)), tag
        m = r.model
        assert m.arith_ == ("reference" if orc.device_arith(n, ob.cluster_centers_.size)[0] == "A" else "fixed"), tag
        assert m.n_iter_ == ob.n_iter_, (tag, m.n_iter_, ob.n_iter_)
        assert np.array_equal(_u32(m.cluster_centers_.ravel()), _u32(ob.cluster_centers_.ravel())), tag
        assert np.array_equal(m.labels_, ob.labels_), (tag, int((m.labels_ != ob.labels_).sum()))
        assert np.array_equal(_u32(r.values.cpu().numpy()), _u32(ob.cluster_centers_.ravel()[ob.labels_])), tag
        assert np.array_equal(r.counts, counts) and np.array_equal(r.code_lengths, lengths) and r.total_bits == total, tag
        assert np.array_equal(r.length_hist, lhist), tag
        events, multi, _, _ = _summary(ob)
        assert m.n_relocations_ == events and m.n_reloc_multi_ == multi, (tag, m.n_relocations_, events, m.n_reloc_multi_, multi)
        _check_tie_report(m, ob, tag)


def test_the_two_extra_pruned_inputs_give_the_references_outcome(nnc):
    """Nearly everything pruned, and fewer non-zero weights than centres: the reference raises nothing and returns a fit (recorded
    with the goldens); the reference's surface on the device does the same and, in the reference's arithmetic with NumPy's own
    selection at the ties these fits are full of, returns the reference's result bit for bit."""
    for name, n, q in (shapes.FEWER_NONZERO_THAN_CENTRES, shapes.NEARLY_ALL_PRUNED):
        i = G.inputs[shapes.input_key(name, n, q)]
        assert i["n_nonzero"] < 16
        for mode in ("linear", "density"):
            c = G.cases[shapes.fit_key(name, n, q, mode, 4)]
            assert "raises" not in c
            w = shapes.make(name, n)
            mask = nnc.utility.prune_weigth(w, threshold=q, std_smooth=True)
            assert shapes.sha(np.packbits(mask.ravel())) == i["mask_sha256"]
            cdfs = nnc.utility.get_weight_distribution(w[w != 0]) if mode == "density" else None
            qw, km = nnc.utility.get_quantized_weight(w.copy(), bits=4, mode=mode, cdfs=cdfs, arith="reference", reloc="reference")
            assert km.n_iter_ == c["n_iter"]
            assert np.array_equal(_u32(km.cluster_centers_.ravel()), _u32(G.centers(c)))
            assert shapes.sha(km.labels_.astype(np.int32)) == c["labels_sha256"]
            assert np.array_equal(qw, km.cluster_centers_[km.labels_].reshape(w.shape))
            qd, kd = nnc.utility.get_quantized_weight(w.copy(), bits=4, mode=mode, cdfs=cdfs)       # the default: no exception either
            assert kd is not None and np.array_equal(qd, kd.cluster_centers_[kd.labels_].reshape(w.shape))


# ------------------------------------------------------------------ i. downstream of such a fit
@pytest.mark.parametrize("name", ["outliers", "ternary"])
def test_downstream_of_a_fit(nnc, name, tmp_path):
    """Index coding, storage and the codebook matmul on fits whose index histograms are as lopsided as they get (the bulk in one or
    two clusters, clusters of one member, clusters that stayed empty)."""
    from tests.helpers import cbmm_ref

    key = shapes.fit_key(name, 50_000, None, "linear", 4)
    c = G.cases[key]
    x = dev(shapes.case_input(c))
    model, vals = nnc.kmeans.DeviceKMeans(x, G.init(c)).fit()
    ob = oracle_fit(key, "B")
    k = c["K"]
    want = ob.cluster_centers_.ravel()[ob.labels_]
    assert np.array_equal(model.labels_, ob.labels_)
    # Huffman encode / decode of the indices
    words, chunk_bits, lengths, total_bits = nnc.storage.encode_indices(model.labels_compact_, k)
    ol, _, ot = orc.huffman_lengths(np.bincount(ob.labels_, minlength=k))
    assert total_bits == ot and np.array_equal(lengths, ol)
    back = nnc.storage.decode_indices(words, chunk_bits, c["n"], lengths, k, 1)
    assert torch.equal(back, model.labels_compact_)
    # save / load
    path = str(tmp_path / "t.nnc")
    kdim, ncols = 250, 200
    nnc.storage.save_compressed(path, {"w": ((kdim, ncols), model, None)})
    loaded = nnc.storage.load_compressed(path)["w"]
    assert loaded.shape == (kdim, ncols) and np.array_equal(_u32(loaded.cpu().numpy().ravel()), _u32(want))
    # the layer run from codebook + indices, against a float64 matmul
    cen = dev(model.cluster_centers_.ravel())
    layer = nnc.compressed.CompressedDense(kdim, ncols, model.labels_compact_, cen, None)      # (its constructor is the from-codes form)
    wm = want.reshape(kdim, ncols)
    for m in (1, 17):
        xin = shapes.make("cubic", m * kdim).reshape(m, kdim) * np.float32(8)
        with torch.no_grad():
            y = layer(dev(xin)).cpu().numpy()
        y64 = cbmm_ref.matmul64(xin, wm)
        mag = np.abs(xin.astype(np.float64)) @ np.abs(wm.astype(np.float64))
        bound = 2.0 * kdim * 2.0 ** -24 * mag + 1e-30      # (the float32 bound of the codebook matmul tests)
        assert np.all(np.abs(y.astype(np.float64) - y64) <= bound), (name, m, float((np.abs(y - y64) / bound).max()))
