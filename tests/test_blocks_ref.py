"""The references and case data of tests/helpers/blocks_ref.py, checked on the CPU: the cases hold the edges they name, the
selection distributions stop at the refinement levels they claim, and the references agree with plainer forms of themselves."""
import numpy as np
import pytest

from tests.helpers import blocks_ref as br


def test_lengths():
    ls = br.small_lengths()
    assert ls == [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 8191, 8193, 70_001]
    assert br.big_length(256) == 256 * 8 * 1024 + 4099 and br.big_length(256) % 4 != 0


@pytest.mark.parametrize("inf,nan", [(False, False), (True, False), (True, True)])
def test_special_values_are_present(inf, nan):
    for n in br.small_lengths():
        x = br.special_f32(n, 3 + n, inf=inf, nan=nan)
        assert x.dtype == np.float32 and x.size == n
        assert np.array_equal(br.bits(x), br.bits(br.special_f32(n, 3 + n, inf=inf, nan=nan)))   # seeded
        if n < 64:
            continue
        u = br.bits(x)
        want = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF]
        if inf:
            want += [0x7F800000, 0xFF800000]
        if nan:
            want += [0x7FC00000, 0xFFC12345, 0x7F800001]
        for w in want:
            assert np.count_nonzero(u == w) >= 2, (n, hex(w))
        assert np.isnan(x).any() == nan and np.isinf(x).any() == inf
        if n >= 255:
            assert np.any(x[1:] == x[:-1])          # a run of equal values
    x = br.special_f32(1025, 1, huge=False)
    assert np.abs(x).max() < 1.0


def test_ordered_bits_is_strictly_increasing():
    vals = np.array([-np.inf, -br.FLT_MAX, -1.5, -1.0, -br.NORMAL_MIN, -br.SUBNORMAL_MIN, -0.0, 0.0, br.SUBNORMAL_MIN,
                     br.NORMAL_MIN, 1.0, np.nextafter(np.float32(1), np.float32(2)), 1.5, br.FLT_MAX, np.inf], dtype=np.float32)
    ob = br.ordered_bits(vals).astype(np.int64)
    assert np.all(np.diff(ob) > 0)
    assert ob[6] == 0x7FFFFFFF and ob[7] == 0x80000000           # -0.0 directly below +0.0
    rng = np.random.RandomState(0)
    x = np.unique(rng.standard_normal(5000).astype(np.float32))
    assert np.all(np.diff(br.ordered_bits(x).astype(np.int64)) > 0)
    k = br.key64(np.array([0.25, 0.25, 0.5], dtype=np.float32), np.array([1.0, -1.0, -5.0], dtype=np.float32))
    assert k.dtype == np.int64 and k[2] > k[0] > k[1] > 0
    assert k[0] == (0x3E800000 << 32) | 0xBF800000


def test_top_keys_ref_tells_the_zeros_apart():
    d = np.full(4, 0.5, dtype=np.float32)
    x = np.array([-0.0, 0.0, -0.0, -1.0], dtype=np.float32)
    keys = br.top_keys_ref(d, x, 2)
    assert keys.size == 3 and np.array_equal(keys & 0xFFFFFFFF, [0x80000000, 0x7FFFFFFF, 0x7FFFFFFF])
    assert br.top_keys_ref(d, x, 7).size == 4


@pytest.mark.parametrize("name", sorted(br.SELECTION_STOPS))
def test_selection_distributions_stop_where_claimed(name):
    d = br.selection_distances()[name]
    assert d.dtype == np.float32 and d.size == br.SELECTION_N and np.all(d >= 0)
    for m in br.SELECTION_M:
        used, cand, fallback = br.levels_ref(d, m)
        assert (used, fallback) == br.SELECTION_STOPS[name][m], (name, m, used, cand, fallback)
        assert cand >= m + 1
        if name == "one_prefix":
            assert 1000 < cand < 2500, cand
        if fallback:
            assert cand == br.SELECTION_N > br.TOPM_CAP
    u = br.bits(d)
    if name == "one_bin":
        assert np.unique(u >> 19).size <= 2 and np.bincount((u >> 19) - (u >> 19).min()).max() > br.TOPM_CAP
    if name == "one_prefix":
        assert np.unique(u >> 7).size == 1 and np.unique(u).size == 128
    if name == "crowd":
        assert np.count_nonzero(d != 0.25) == 5 and np.unique(d).size == 6


def test_selection_values_hold_both_zeros_and_duplicates():
    x = br.selection_values()
    u = br.bits(x)
    assert (u == 0).any() and (u == 0x80000000).any() and (x < 0).any() and np.unique(u).size < 200


def test_hist_cases_hold_their_edges():
    cases = br.hist_cases()
    assert set(cases) == {"a_special_huge", "a_special", "b_on_every_step", "c_repeated_steps", "d_constant", "e_zeros_counted",
                          "e_zeros_skipped", "f_outside"}
    for name, (x, steps, skip) in cases.items():
        assert x.dtype == np.float32 and steps.dtype == np.float32 and steps.size == 32 and x.size > 0, name
        assert np.all(np.diff(steps) >= 0), name
        # the ranks of the steps in the sorted vector give the same histogram (NaN sorts last and is in no bin)
        xs = np.sort(x[x != 0] if skip else x)
        assert np.array_equal(np.diff(br.rank_ref(xs, steps)), br.hist31_ref(x, steps, skip)), name
    x, steps, _ = cases["b_on_every_step"]
    h = br.hist31_ref(x, steps, False)
    for b in range(32):
        assert np.count_nonzero(x == steps[b]) == 3, b
    only = br.hist31_ref(np.repeat(steps, 3), steps, False)
    assert np.array_equal(only, np.full(31, 3))                        # step b lands in bin b, the last step in none
    assert h.sum() == x.size - 3
    x, steps, _ = cases["c_repeated_steps"]
    assert np.unique(x).size == 6 and np.unique(steps).size == 6 and np.any(np.diff(steps) == 0)
    h = br.hist31_ref(x, steps, False)
    assert sorted(h.tolist()) == [0] * 26 + [10] * 5
    x, steps, _ = cases["d_constant"]
    assert np.unique(x).size == 1 and np.all(steps == x[0]) and not br.hist31_ref(x, steps, False).any()
    x, steps, _ = cases["e_zeros_counted"]
    nzero = np.count_nonzero(x == 0)
    assert (br.bits(x) == 0).any() and (br.bits(x) == 0x80000000).any() and not np.any(steps == 0)
    diff = br.hist31_ref(x, steps, False) - br.hist31_ref(x, steps, True)
    assert diff.sum() == nzero and np.count_nonzero(diff) == 1
    x, steps, _ = cases["f_outside"]
    assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
    with np.errstate(invalid="ignore"):
        inside = np.count_nonzero((x >= steps[0]) & (x < steps[31]))
        assert np.any(x < steps[0]) and np.any(x > steps[31])
    assert br.hist31_ref(x, steps, False).sum() == inside < x.size


def test_rank_values_hold_their_edges():
    xs = np.sort(br.special_f32(1025, 5, huge=False, inf=False))
    xs[xs == 0] = 0.0                                                   # a run of +0.0 only
    edge = br.rank_edge_values(xs)
    assert (br.bits(edge) == 0x80000000).any() and np.isinf(edge).sum() == 2
    assert edge.min() < xs[0] and edge.max() > xs[-1]
    r = br.rank_ref(xs, edge)
    assert r.min() == 0 and r.max() == xs.size
    z = np.nonzero(xs == 0)[0]
    assert z.size >= 2 and br.rank_ref(xs, np.float32(-0.0)) == z[0] == br.rank_ref(xs, np.float32(0.0))
    # a member of a run of duplicates ranks at the start of its run: "<=" instead of "<" would give its end
    dup = xs[1:][xs[1:] == xs[:-1]]
    assert dup.size and np.any(np.searchsorted(xs, edge, side="right") != r)
    for ys in (xs, np.sort(br.special_f32(1025, 6, inf=True)), np.zeros(1, dtype=np.float32)):
        for m in (1, 32, 64, 65, 200):
            v = br.rank_values(ys, m)
            assert v.size == m and v.dtype == np.float32 and not np.isnan(v).any()


def test_ref_sums_ref_equals_a_python_loop():
    x, l = br.ref_sums_case(257, 6, 1, 2)
    for mean in (0.0, 0.0125):
        sums, counts = br.ref_sums_ref(x, mean, l, 6)
        want = [np.float32(0.0)] * 6
        cnt = [0] * 6
        for xi, li in zip(x, l):
            if li < 6:
                want[li] = np.float32(want[li] + np.float32(xi - np.float32(mean)))
                cnt[li] += 1
        assert np.array_equal(br.bits(sums), br.bits(np.array(want, dtype=np.float32))), mean
        assert counts.tolist() == cnt
    sums, counts = br.ref_sums_ref(x, 0.0, l, 6)
    assert counts[1] == counts[3] == counts[5] == 0 and counts[0] > 0 and counts[2] > 4 and (l >= 6).any()
    assert np.all(br.bits(x[l == 0]) == 0x80000000)
    assert br.bits(sums)[0] == 0 and br.bits(sums)[1] == 0              # the -0.0 cluster and an empty one sum to +0.0
    # the order decides: the running float32 sum loses the 1 that follows 1e8, the exact sum of the same terms does not
    v = x[l == 2]
    assert np.float32(v.astype(np.float64).sum()) != sums[2]
    # without the leading +0.0 the cluster of -0.0 terms would come out as -0.0
    assert br.bits(np.cumsum(x[l == 0], dtype=np.float32)[-1:])[0] == 0x80000000


def test_label_cases_and_small_references():
    for lb, k in ((1, 1), (1, 16), (1, 255), (1, 256), (2, 257), (2, 1040)):
        l = br.labels_with_outliers(1025, k, lb, k)
        assert l.dtype == (np.uint8 if lb == 1 else np.uint16)
        top = 255 if lb == 1 else 65535
        if k <= top:
            assert (l == k).any() and (l == top).any()
        c = br.bincount_ref(l, k)
        assert c.size == k and c.sum() == np.count_nonzero(l.astype(np.int64) < k)
        assert np.array_equal(br.bincount_ref(l.view(np.int8 if lb == 1 else np.int16), k), c)      # signed storage reads as unsigned
        centers = br.from_bits(np.arange(k, dtype=np.uint32) + np.uint32(0x80000000))              # -0.0, negative subnormals
        g = br.gather_ref(centers, l)
        ok = l.astype(np.int64) < k
        assert np.array_equal(br.bits(g)[ok], l[ok].astype(np.uint32) + np.uint32(0x80000000)) and not br.bits(g)[~ok].any()


def test_minmax_and_threshold_references():
    x = np.array([0.0, -0.0, np.nan, -br.SUBNORMAL_MIN, 2.0, -np.inf], dtype=np.float32)
    assert br.minmax_ref(x) == (-np.inf, 2.0, -np.inf, 2.0, 2, 2, 6)
    assert br.minmax_ref(x, True)[6] == 4
    x = br.special_f32(63, 104, nan=True)                                # NaN next to the extremes: skipped, not contagious
    assert np.isnan(x).any() and br.minmax_ref(x)[:4] == (-br.FLT_MAX, br.FLT_MAX, -br.FLT_MAX, br.FLT_MAX)
    z = np.array([0.0, -0.0], dtype=np.float32)
    assert br.minmax_ref(z, True) == (np.inf, -np.inf, np.inf, -np.inf, 0, 2, 0)
    assert br.minmax_ref(np.array([0.0, -3.0, 0.0], dtype=np.float32), True)[:4] == (-3.0, -3.0, -3.0, -3.0)
    x = br.from_bits(np.array([0x80000000, 0x00000001, 0x3F800000, 0xBF800000, 0x7FC00001, 0xFF800000, 0x3F7FFFFF], dtype=np.uint32))
    out, mask = br.threshold_ref(x, 1.0)
    assert mask.tolist() == [1, 1, 0, 0, 0, 0, 1]                       # strict: +-thr survive; NaN and inf survive
    assert br.bits(out).tolist() == [0, 0, 0x3F800000, 0xBF800000, 0x7FC00001, 0xFF800000, 0]
    out, mask = br.threshold_ref(x, 0.0)
    assert not mask.any() and np.array_equal(br.bits(out), br.bits(x))  # nothing is below 0: -0.0 keeps its sign
    out, mask = br.threshold_ref(x, np.inf)
    assert mask.tolist() == [1, 1, 1, 1, 0, 0, 1]


def test_topm_hist_ref():
    d = br.from_bits(np.array([0, 1, 0x7F7FFFFF, 0x7F800000, 0x3E800000, 0x3E80007F], dtype=np.uint32))
    h = br.topm_hist_ref(d, 19, 12, -1, 0)
    assert h.size == 4096 and h.sum() == 6 and h[0] == 2 and h[0x7F7FFFFF >> 19] == 1 and h[0x7F800000 >> 19] == 1 and h[0x3E800000 >> 19] == 2
    h = br.topm_hist_ref(d, 0, 7, 7, 0x3E800000 >> 7)
    assert h.sum() == 2 and h[0] == 1 and h[127] == 1
    assert br.topm_hist_ref(d, 31, 1, -1, 0)[0] == 6
