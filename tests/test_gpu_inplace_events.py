"""Empty-cluster events of a chosen size, settled where the iteration runs (csrc/nnc_lloyd.hpp, kl_relocate: the candidate keys stay in
registers, every thread keeps its m + 1 largest, the waves and then the workgroup merge the lists) -- by the resident loop (k_lloyd) and
by the finalize step of the launch-per-iteration pair (km_finalize_relocate).  The yardstick is the oracle in mode B; the two device
forms are held against each other and against it bit for bit: n_iter_, centres, labels, decoded values, the number of events, of events
with several empty clusters, and the tie report.

Inputs: a sigma-pruned tensor, K - m distinct quantiles of its NON-zero weights (the plateau of zeros would make duplicates by itself)
and m copies of one of them -- lowest, middle or highest.  The copies own nothing, so iteration 0 has an event of exactly m empty
clusters (the oracle's trace says so, and the tests read the sizes from there, not from m).

Reference path: _relocate_empty_clusters_dense (sklearn/cluster/_k_means_common.pyx:167-211), reached from KMeans.fit as called in
neural_network_compression/common/utility.py:237-238."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from neural_network_compression_amd import synth  # noqa: E402
from oracle import oracle as orc  # noqa: E402

RM_MAX = 7   # KL_RM_MAX (csrc/nnc_lloyd.hpp): the largest event kl_relocate takes; one of RM_MAX + 1 is handed on


@pytest.fixture(scope="module")
def km():
    assert torch.cuda.is_available()
    from neural_network_compression_amd import _native, build as _b, kmeans
    _b.build_native()
    _native.load()
    return kmeans


def _pruned(n, seed):
    x = synth.weights((n,), seed)
    orc.prune_weigth(x, 1.0, True)
    return x


def _with_copies(x, k, m, where):
    """k - m distinct quantiles of the non-zero values of x, then m copies of the lowest / middle / highest of them."""
    nz = x[x != 0].astype(np.float64)
    base = np.unique(np.quantile(nz, np.linspace(0.002, 0.998, k - m)).astype(np.float32))
    assert base.size == k - m
    dup = {"lowest": base[0], "middle": base[base.size // 2], "highest": base[-1]}[where]
    return np.concatenate([base, np.full(m, dup, dtype=np.float32)]).astype(np.float32)


def sized(n, k, m, where, seed):
    x = _pruned(n, seed)
    return x, _with_copies(x, k, m, where)


def few_valued(n, k, m, where, seed, levels=64):
    """Weights rounded to `levels` values: the farthest samples are copies of one value, so two moved centres land on the same value --
    the order ties by original index and the table of distinct centres shrinks."""
    x = _pruned(n, seed)
    step = np.float32((x.max() - x.min()) / levels)
    x = (np.round(x / step) * step).astype(np.float32)
    vals = np.unique(x[x != 0])
    base = vals[np.round(np.linspace(0, vals.size - 1, k - m)).astype(int)]
    assert np.unique(base).size == k - m
    dup = {"lowest": base[0], "middle": base[base.size // 2], "highest": base[-1]}[where]
    return x, np.concatenate([base, np.full(m, dup, dtype=np.float32)]).astype(np.float32)


def outliers(n, k, m, seed, copies=12):
    """`copies` equal outliers beyond the upper tail: more of the largest keys sit at the upper end of the last stretch than an end
    supplies candidates (8), all equally far, so the innermost candidate is not strictly below the cut and the proof refuses."""
    x = _pruned(n, seed)
    init = _with_copies(x, k, m, "middle")
    x[:: n // copies][:copies] = np.float32(3.0) * x.max()
    return x, init


def lone_outlier(n, k, m, seed):
    """One sample far above everything with a centre of its own that does not sit on it: the farthest sample of iteration 0 is the
    only one of its cluster, and taking it would leave that cluster empty."""
    x = _pruned(n, seed)
    init = _with_copies(x, k, m + 1, "middle")
    top = np.float32(10.0) * x.max()
    x[n // 2] = top
    init[k - 1] = np.float32(0.8) * top   # (one copy becomes the outlier's centre: m copies stay)
    return x, init


def all_equal(n, k, m, seed):
    x = np.full(n, -0.375, dtype=np.float32)
    init = np.linspace(-0.375, 0.5, k - m).astype(np.float32)
    return x, np.concatenate([init, np.full(m, -0.375, dtype=np.float32)]).astype(np.float32)


# name -> (builder, arguments).  K = 8 / 24 / 33 / 64: the loop is the library's own choice (256 threads); 65 / 129: the loop forced
# (256 threads) and the pair; 257 / 300: the pair and the loop forced (1024 threads).  Every case runs both forms.
CASES = {
    "k257_m1_middle": (sized, (30_000, 257, 1, "middle", 11)),
    "k257_m2_lowest": (sized, (30_000, 257, 2, "lowest", 12)),
    "k257_m7_highest": (sized, (30_000, 257, 7, "highest", 13)),
    "k257_m8_middle": (sized, (30_000, 257, 8, "middle", 14)),
    "k64_m3_middle": (sized, (20_000, 64, 3, "middle", 15)),
    "k24_m7_lowest": (sized, (20_000, 24, 7, "lowest", 16)),
    "k129_m5_highest": (sized, (40_000, 129, 5, "highest", 17)),
    "k65_m1_lowest": (sized, (40_000, 65, 1, "lowest", 18)),
    "k8_m2_middle": (sized, (20_000, 8, 2, "middle", 19)),
    "k33_m1_highest": (sized, (20_000, 33, 1, "highest", 20)),
    "k300_m4_middle": (sized, (60_000, 300, 4, "middle", 21)),
    "few_valued_k24_m2": (few_valued, (20_000, 24, 2, "middle", 22)),
    "few_valued_k129_m3": (few_valued, (40_000, 129, 3, "lowest", 23, 512)),
    "outliers_k33_m2": (outliers, (20_000, 33, 2, 24)),
    "outliers_k257_m3": (outliers, (30_000, 257, 3, 25)),
    "lone_outlier_k16_m1": (lone_outlier, (20_000, 16, 1, 26)),
    "lone_outlier_k257_m2": (lone_outlier, (30_000, 257, 2, 27)),
    "all_equal_k8_m3": (all_equal, (5_000, 8, 3, 28)),
}

_oracle_cache = {}


def oracle_fit(name):
    """(x, init, oracle fit with its trace), computed once a case."""
    if name not in _oracle_cache:
        fn, args = CASES[name]
        x, init = fn(*args)
        _oracle_cache[name] = (x, init, orc.kmeans_lloyd(x, init, accum="B", keep_trace=True))
    return _oracle_cache[name]


def event_sizes(ob):
    return [t["n_empty"] for t in ob.trace if t["n_empty"]]


_runs = {}


def _run(km, name):
    """Both device forms against each other and against the oracle; returns what the summary test adds up."""
    if name in _runs:
        return _runs[name]
    x, init, ob = oracle_fit(name)
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    a_km = km.DeviceKMeans(t, init, loop=True)
    assert a_km.lloyd, "the one-workgroup loop must be the path taken"
    b_km = km.DeviceKMeans(t, init, two_launch=True)
    assert not b_km.lloyd
    a, av = a_km.fit()
    b, bv = b_km.fit()
    info = ob.reloc_info_
    events, multi = int(info.get("reloc_events", 0)), int(info.get("reloc_multi", 0))
    distinct, any_tie = int(info.get("reloc_ties_distinct", 0)), int(info.get("reloc_ties", 0))
    in_place = {}
    for tag, d, m_, v in (("loop", a_km, a, av), ("pair", b_km, b, bv)):
        st = d.loop_stats()
        in_place[tag] = st["relocated_in_loop"]
        print(f"{name} [{tag}]: n_iter {m_.n_iter_}/{ob.n_iter_}; events {m_.n_relocations_}/{events} (sizes {event_sizes(ob)}), multi {m_.n_reloc_multi_}/{multi}, "
              f"tie {m_.reloc_tie_}/{distinct} of {any_tie}; settled in place {st['relocated_in_loop']}, passed on why {st['passed_on_why']}")
        assert m_.n_iter_ == ob.n_iter_, (name, tag, m_.n_iter_, ob.n_iter_)
        assert np.array_equal(m_.cluster_centers_.ravel().view(np.uint32), ob.cluster_centers_.ravel().view(np.uint32)), (name, tag)
        assert np.array_equal(m_.labels_, ob.labels_), (name, tag)
        assert np.array_equal(v.cpu().numpy().view(np.uint32), ob.cluster_centers_.ravel()[ob.labels_].view(np.uint32)), (name, tag)
        assert m_.n_relocations_ == events, (name, tag, m_.n_relocations_, events)
        assert m_.n_reloc_multi_ == multi, (name, tag, m_.n_reloc_multi_, multi)
        assert (m_.reloc_tie_ != 0) == (distinct != 0) and m_.reloc_tie_ <= any_tie, (name, tag, m_.reloc_tie_, distinct, any_tie)
        assert 0 <= st["relocated_in_loop"] <= m_.n_relocations_, (name, tag, st)
    assert (a.n_iter_, a.stop_reason_, a.n_relocations_, a.reloc_tie_, a.n_reloc_multi_) == (b.n_iter_, b.stop_reason_, b.n_relocations_, b.reloc_tie_, b.n_reloc_multi_), name
    assert np.array_equal(a.cluster_centers_.view(np.uint32), b.cluster_centers_.view(np.uint32)), name
    assert np.array_equal(a.labels_, b.labels_) and torch.equal(av, bv), name
    _runs[name] = {"sizes": event_sizes(ob), "events": events, "in_place": in_place}
    return _runs[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_event_same_trajectory_in_both_forms(km, name):
    _run(km, name)


def test_first_event_has_the_size_asked_for():
    """The recipe does what it says (oracle only): iteration 0 of every `sized` case has exactly m empty clusters, the events of the
    file cover 1, 2, KL_RM_MAX and KL_RM_MAX + 1, and every edge is really hit."""
    seen = set()
    for name, (fn, args) in CASES.items():
        _, init, ob = oracle_fit(name)
        tr = ob.trace
        seen.update(event_sizes(ob))
        if fn is sized:
            assert tr[0]["n_empty"] == args[2], (name, tr[0]["n_empty"])
    assert {1, 2, RM_MAX, RM_MAX + 1} <= seen, sorted(seen)
    # lowest / highest copy: the moved centres leave rank 0 / K - 1 of the order (the copies tie there by index)
    for name, end in (("k257_m2_lowest", 0), ("k257_m7_highest", -1), ("k65_m1_lowest", 0), ("k33_m1_highest", -1)):
        _, init, _ = oracle_fit(name)
        assert init[-1] == np.sort(init)[end], name
    # two moved centres next to each other in the order behind the event
    _, init, ob = oracle_fit("k257_m2_lowest")
    rank = np.argsort(np.argsort(ob.trace[0]["centers"], kind="stable"), kind="stable")
    assert abs(int(rank[-1]) - int(rank[-2])) == 1, rank[-2:]
    # few-valued data: two moved centres land on one value
    _, init, ob = oracle_fit("few_valued_k24_m2")
    c0 = ob.trace[0]["centers"]
    assert c0[-1] == c0[-2] and np.unique(c0).size < c0.size
    # equal outliers: at least nine samples tie at the top distance of iteration 0 (an end supplies eight candidates)
    for name in ("outliers_k33_m2", "outliers_k257_m3"):
        x, init, ob = oracle_fit(name)
        assert int((x == x.max()).sum()) >= 9 and ob.trace[0]["n_empty"] >= 1, name
    # the lone outlier is taken in iteration 0 and leaves its cluster without a sample
    for name in ("lone_outlier_k16_m1", "lone_outlier_k257_m2"):
        x, init, ob = oracle_fit(name)
        assert ob.trace[0]["n_empty"] >= 1 and int((ob.trace[0]["counts"] == 0).sum()) >= 1, (name, ob.trace[0]["counts"])
    # all-equal data: one centre owns everything, every sample sits on it, nothing to move
    _, init, ob = oracle_fit("all_equal_k8_m3")
    assert ob.trace[0]["n_empty"] == init.size - 1 and ob.reloc_info_.get("reloc_events", 0) == 0


def test_events_are_settled_in_place_in_both_forms(km):
    """Summed over the file: both the loop and the finalize step of the pair settled events themselves; an event of KL_RM_MAX + 1 was
    met (and, as every case asserts, gave the oracle's trajectory)."""
    loop = pair = events = 0
    seen = set()
    for name in sorted(CASES):
        r = _run(km, name)
        loop += r["in_place"]["loop"]
        pair += r["in_place"]["pair"]
        events += r["events"]
        seen.update(r["sizes"])
    print(f"events {events}, settled in place: loop {loop}, pair {pair}; sizes {sorted(seen)}")
    assert {1, 2, RM_MAX, RM_MAX + 1} <= seen, sorted(seen)
    assert events > 0 and loop > 0 and pair > 0, (events, loop, pair)
