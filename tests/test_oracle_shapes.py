"""Pin the CPU oracle to what the reference itself produced on heavy-tailed, offset and few-valued weights
(tests/helpers/shapes.py; goldens tests/golden/ref_shapes.*, made by tests/golden/make_goldens_shapes.py).  No GPU needed.

Mode A of the oracle equals the reference bit for bit on every golden: masks, weight distributions, initial centres, n_iter_,
centres, indices.  The gap to the device's arithmetic (stored with each case, computed on the CPU) sorts the fits into tight /
summation / divergent with the project's two existing ceilings; the divergent ones are listed by key with their cause."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.helpers import ab_gap, shapes

G = shapes.goldens()


def test_recipes_are_reproduced_bit_for_bit():
    assert len(G.inputs) == 2 * 3 * len(shapes.SHAPES) + 2
    for ikey, i in G.inputs.items():
        w = shapes.make(i["shape"], i["n"])
        assert w.dtype == np.float32 and shapes.sha(w) == i["input_sha256"], ikey
    # what each recipe is for
    assert shapes.make("gain", 3000).min() > 0.8 and shapes.make("onesided", 3000).min() >= 0 and shapes.make("negative", 3000).max() <= 0
    assert set(np.unique(shapes.make("ternary", 3000))) == {np.float32(-0.125), np.float32(0.0), np.float32(0.125)}
    o = shapes.make("outliers", 50_000)
    assert np.abs(o).max() > 40 * np.sort(np.abs(o))[-9] and np.std(o) > 4 * np.std(np.sort(np.abs(o))[:-8])


@pytest.mark.parametrize("ikey", sorted(G.inputs))
def test_statistics_mask_and_distribution_equal_the_reference(ikey):
    i = G.inputs[ikey]
    w = shapes.make(i["shape"], i["n"])
    assert shapes.f32_bits(orc.np_mean(w)) == i["mean_bits"] and shapes.f32_bits(orc.np_var(w)) == i["var_bits"]
    assert shapes.f32_bits(orc.np_std(w)) == i["sigma_bits"] == shapes.f32_bits(np.std(w))
    if i["q"] is not None:
        mask = orc.prune_weigth(w, i["q"], True)
        assert int(mask.sum()) == i["nzeroed"] and shapes.sha(np.packbits(mask.ravel())) == i["mask_sha256"]
        assert np.array_equal(mask, np.abs(shapes.make(i["shape"], i["n"])) < np.std(shapes.make(i["shape"], i["n"])) * i["q"])
    nz = w[w != 0]
    assert nz.size == i["n_nonzero"]
    xnew, cdf = orc.get_weight_distribution(nz)
    gx, gc = G.cdfs(i)
    assert str(xnew.dtype) == G.manifest["dtypes"]["xnew"] and str(cdf.dtype) == G.manifest["dtypes"]["cdf"]
    assert np.array_equal(xnew.view(np.uint32), gx.view(np.uint32)) and np.array_equal(cdf.view(np.uint64), gc.view(np.uint64))
    assert int(np.unique(cdf).size) == i["cdf_distinct"]


def test_the_two_extra_pruned_inputs():
    name, n, q = shapes.FEWER_NONZERO_THAN_CENTRES
    assert G.inputs[shapes.input_key(name, n, q)]["n_nonzero"] < 16                       # fewer non-zero weights than centres
    name, n, q = shapes.NEARLY_ALL_PRUNED
    i = G.inputs[shapes.input_key(name, n, q)]
    assert i["nzeroed"] > 0.999 * n and i["n_nonzero"] >= 1                                # sigma is the spikes', the bulk goes
    for mode, bits in shapes.MODES:                                                        # the reference fits them all the same, with a warning
        for key in (shapes.fit_key(*shapes.FEWER_NONZERO_THAN_CENTRES, mode, bits), shapes.fit_key(*shapes.NEARLY_ALL_PRUNED, mode, bits)):
            c = G.cases[key]
            assert "raises" not in c and "n_iter" in c
            if 2 ** bits > 9:
                assert [m[0] for m in G.messages(c)] == ["ConvergenceWarning"], key


@pytest.mark.parametrize("key", G.fits())
def test_oracle_mode_a_is_the_reference_bit_for_bit(key):
    c = G.cases[key]
    w = shapes.case_input(c)
    i = G.input_of(c)
    if c["q"] is None:
        assert shapes.sha(w) == i["input_sha256"]
    cdfs = None
    if c["mode"] == "density":
        cdfs = orc.get_weight_distribution(w[w != 0])
    if c["forgy_seed"] is not None:
        np.random.seed(c["forgy_seed"])
    init = np.asarray(orc.init_space(w, c["bits"], c["mode"], cdfs), dtype=np.float32)
    assert np.array_equal(init.view(np.uint32), G.init(c).view(np.uint32)), key
    assert int(np.unique(init).size) == c["init_distinct"]
    kw = {} if c["max_iter"] is None else {"max_iter": c["max_iter"]}
    km = orc.kmeans_lloyd(w, init, accum="A", **kw)
    assert km.n_iter_ == c["n_iter"], (key, km.n_iter_, c["n_iter"])
    assert np.array_equal(km.cluster_centers_.ravel().view(np.uint32), G.centers(c).view(np.uint32)), key
    assert shapes.sha(km.labels_.astype(np.int32)) == c["labels_sha256"], key
    assert np.array_equal(np.bincount(km.labels_, minlength=c["K"]), G.bincount(c)), key
    assert {k: int(v) for k, v in km.reloc_info_.items()} == c["reloc_A"], key
    if c["max_iter"] is not None:
        assert km.n_iter_ == c["max_iter"]


def test_what_the_inputs_exercise():
    """The data-dependent events the older goldens hardly have are all over these: relocation events, several clusters empty at
    once, ties at the cut, initial centres with duplicates (a flat CDF), long fits, the iteration cap."""
    fits = [G.cases[k] for k in G.fits()]
    assert len(fits) >= 220 and not G.dropped
    assert sum(1 for c in fits if c["reloc_dev"].get("reloc_events", 0)) >= 100
    assert sum(1 for c in fits if c["reloc_dev"].get("reloc_multi", 0)) >= 80
    assert sum(1 for c in fits if c["reloc_dev"].get("reloc_ties", 0)) >= 30
    # ... nearly all of them between equal values (the zeros of a pruned tensor, the three values of `ternary`): harmless, and not
    # what the device reports; a tie between two different values is rare
    assert 1 <= sum(1 for c in fits if c["reloc_dev"].get("reloc_ties_distinct", 0)) <= 5
    assert all(c["reloc_dev"].get("reloc_ties_distinct", 0) <= c["reloc_dev"].get("reloc_ties", 0) for c in fits)
    assert sum(1 for c in fits if c["n_iter"] > 100) >= 5 and max(c["n_iter"] for c in fits) <= shapes.MAX_REF_ITER
    dens = [c for c in fits if c["mode"] == "density"]
    assert sum(1 for c in dens if c["shape"] in ("outliers", "quintic") and c["init_distinct"] < c["K"] - 2) >= 10
    assert all(c["init_distinct"] == 1 for c in dens if c["shape"] == "ternary")            # one value repeated
    assert {c["K"] for c in fits} >= {4, 16, 17, 33, 129, 257, 32}


def test_categories_and_the_listed_divergent_fits():
    cats = {k: shapes.category(G.cases[k]) for k in G.fits()}
    plain = [k for k in cats if G.cases[k]["shape"] != "ternary"]
    divergent = {k for k in plain if cats[k] == "divergent"}
    assert divergent == set(shapes.DIVERGENT), (sorted(divergent - set(shapes.DIVERGENT)), sorted(set(shapes.DIVERGENT) - divergent))
    assert len(divergent) <= shapes.DIVERGENT_CAP * len(plain), (len(divergent), len(plain))
    for k in divergent:
        assert shapes.cause(G.cases[k]) == shapes.DIVERGENT[k], k
    for k in plain:
        c, g = G.cases[k], G.cases[k]["gap"]
        if cats[k] == "tight":
            assert g["n_iter"] == c["n_iter"] and g["err"] <= ab_gap.NORTH_STAR_TOL and g["hist_l1"] == 0
        elif cats[k] == "summation":
            assert g["n_iter"] == c["n_iter"] and g["err"] <= ab_gap.SUMMATION_ERROR_CEILING
        if g["arith"] == "A" and not c["reloc_dev"].get("reloc_multi", 0):
            assert g["err"] == 0.0 and g["labels_differing"] == 0, k          # short tensors: the reference's own arithmetic
    n = {name: sum(1 for k in plain if cats[k] == name) for name in ("tight", "summation", "divergent")}
    tern = [k for k in cats if G.cases[k]["shape"] == "ternary"]
    print(f"shape goldens: {n} of {len(plain)}; ternary: {sum(1 for k in tern if cats[k] == 'divergent')} of {len(tern)} divergent")
    assert n["tight"] >= 100


@pytest.mark.parametrize("key", ["fit/outliers/n50000/qnone/linear4", "fit/gain/n6000/q1/density4", "fit/quintic/n50000/qnone/density5",
                                 "fit/ternary/n6000/qnone/density4", "fit/cubic/n50000/qnone/density5/maxiter20"])
def test_stored_gap_is_what_the_oracle_gives(key):
    """The gap stored with each case is the oracle's own (device arithmetic from the golden init against the golden result):
    recomputed here for one case of each kind, so that the manifest cannot drift from the oracle unnoticed."""
    c = G.cases[key]
    w = shapes.case_input(c)
    kw = {} if c["max_iter"] is None else {"max_iter": c["max_iter"]}
    od = orc.kmeans_lloyd(w, G.init(c), accum="device", **kw)
    g = c["gap"]
    assert od.n_iter_ == g["n_iter"] and ab_gap.centre_err(od.cluster_centers_, G.centers(c)) == g["err"]
    assert int(np.abs(np.bincount(od.labels_, minlength=c["K"]) - G.bincount(c)).sum()) == g["hist_l1"]
    assert {k: int(v) for k, v in od.reloc_info_.items()} == c["reloc_dev"]
