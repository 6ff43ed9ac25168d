"""Plain NumPy references and case data for the small kernels the k-means fit and the pipeline are assembled from
(tests/test_gpu_building_blocks.py; checked on the CPU by tests/test_blocks_ref.py).

Every reference is the contract text of include/nnc.h written out with NumPy, independently of the kernels: integers, bit
patterns and float32 comparisons only, so every comparison with the device is exact.  Nothing here needs a GPU.
"""
from __future__ import annotations

import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
SUBNORMAL_MIN = np.float32(2.0 ** -149)
NORMAL_MIN = np.float32(2.0 ** -126)
TOPM_CAP = 1 << 16                      # DeviceKMeans.TOPM_CAP (asserted equal in the GPU test)
QUARTER_BITS = 0x3E800000               # bits(0.25)
TOPM_LEVELS = ((19, 12, -1), (7, 12, 19), (0, 7, 7))   # (shift, width, prefix_shift) of the three refinement levels


# ---------------------------------------------------------------------------------------------------------------- shared helpers
def small_lengths():
    """float4 bodies and tails, one wave, one workgroup, one NumPy chunk."""
    return [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1025, 8191, 8193, 70_001]


def big_length(cus: int) -> int:
    """Just above the largest grid cap any of these launches uses (cus * 8 workgroups of 256 lanes x 4 elements): every
    grid-stride loop makes a second trip."""
    return int(cus) * 8 * 1024 + 4099


def bits(x) -> np.ndarray:
    """The uint32 bit patterns of a float32 array."""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def from_bits(u) -> np.ndarray:
    return np.ascontiguousarray(u, dtype=np.uint32).view(np.float32)


_FINITE_SPECIALS = [0.0, -0.0, 2.0 ** -149, -(2.0 ** -149), 2.0 ** -126, -(2.0 ** -126)]


def special_f32(n: int, seed: int, huge: bool = True, inf: bool = False, nan: bool = False) -> np.ndarray:
    """Bell-shaped float32 values of scale 0.05 (as synth.weights) with, at seeded positions, runs of equal values and
    +0.0, -0.0, +-2^-149, +-2^-126, +-FLT_MAX (``huge``), +-inf (``inf``) and NaN with a payload (``nan``).  From 64 elements
    on every special value is present at least twice; shorter vectors hold as many as fit."""
    rng = np.random.RandomState(seed)
    x = (rng.standard_normal(n) * 0.05).astype(np.float32)
    for _ in range(max(1, n // 200) if n >= 8 else 0):      # runs of equal values, 2..9 long
        s = rng.randint(0, n - 1)
        x[s:s + rng.randint(2, 10)] = x[s]
    sp = list(_FINITE_SPECIALS)
    if huge:
        sp += [float(FLT_MAX), -float(FLT_MAX)]
    if inf:
        sp += [np.inf, -np.inf]
    spb = list(bits(np.array(sp, dtype=np.float32)))
    if nan:
        spb += [np.uint32(0x7FC00000), np.uint32(0xFFC12345), np.uint32(0x7F800001)]   # quiet, negative with payload, signalling
    reps = max(2, n // 500)
    pos = rng.permutation(n)[: len(spb) * reps]
    u = x.view(np.uint32)
    for i, p in enumerate(pos):
        u[p] = spb[i % len(spb)]
    return x


def ordered_bits(x) -> np.ndarray:
    """The order-preserving uint32 image of float32 (include/nnc.h, the relocation keys): sign bit clear -> bits | 0x80000000,
    sign bit set -> ~bits."""
    b = bits(x)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key64(d, x) -> np.ndarray:
    """bits(d) << 32 | ordered_bits(x), as the int64 the device stores (d >= 0: the top bit is clear)."""
    k = (bits(d).astype(np.uint64) << np.uint64(32)) | ordered_bits(x).astype(np.uint64)
    return k.view(np.int64)


# -------------------------------------------------------------------------------------------------------------------- references
def hist31_ref(x, steps32, skip_zeros: bool) -> np.ndarray:
    """The reference project's per-bin rule, bin by bin, in float32; zeros of both signs removed first when skip_zeros."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    s = np.ascontiguousarray(steps32, dtype=np.float32)
    assert s.size == 32
    if skip_zeros:
        x = x[x != 0]
    with np.errstate(invalid="ignore"):
        return np.array([np.count_nonzero((x >= s[b]) & (x < s[b + 1])) for b in range(31)], dtype=np.int64)


def rank_ref(xs, values) -> np.ndarray:
    """#{ j : xs[j] < values[i] } of an ascending xs."""
    return np.searchsorted(np.ascontiguousarray(xs, dtype=np.float32), np.ascontiguousarray(values, dtype=np.float32),
                           side="left").astype(np.int64)


def _unsigned(labels) -> np.ndarray:
    labels = np.asarray(labels)
    return labels.view({1: np.uint8, 2: np.uint16}[labels.dtype.itemsize]).astype(np.int64)


def bincount_ref(labels, k: int) -> np.ndarray:
    """Labels read as unsigned; an index >= k is not counted."""
    l = _unsigned(labels)
    return np.bincount(l[l < k], minlength=k).astype(np.int64)


def gather_ref(centers, labels) -> np.ndarray:
    """The centre's bits, +0.0 for an index >= k."""
    c = bits(centers)
    l = _unsigned(labels)
    return from_bits(np.where(l < c.size, c[np.minimum(l, c.size - 1)], np.uint32(0)))


def minmax_ref(x, skip_zeros: bool = False):
    """(min, max, min over the non-zeros, max over the non-zeros, #{x < 0}, #{x == 0}, count considered).  min and max
    run over the considered elements (the non-zeros with skip_zeros) and skip NaN as fminf / fmaxf do (+inf / -inf if nothing is
    left); NaN is neither negative nor zero and is counted."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        nz = x[x != 0]
        used = nz if skip_zeros else x
        neg, zer = int(np.count_nonzero(x < 0)), int(np.count_nonzero(x == 0))

    def lo_hi(v):   # (NaN taken out by hand: np.fmin.reduce was seen to return a wrong minimum on a vector that holds NaN)
        v = v[~np.isnan(v)]
        return (v.min(), v.max()) if v.size else (np.float32(np.inf), np.float32(-np.inf))

    return lo_hi(used) + lo_hi(nz) + (neg, zer, int(used.size))


def threshold_ref(x, thr):
    """(pruned x, mask): mask = |x| < thr in float32; a masked element becomes +0.0, every other keeps its bits."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        mask = np.abs(x) < np.float32(thr)
    return from_bits(np.where(mask, np.uint32(0), bits(x))), mask.astype(np.uint8)


def topm_hist_ref(d, shift: int, width: int, pshift: int, prefix: int) -> np.ndarray:
    u = bits(d)
    if pshift >= 0:
        u = u[(u >> np.uint32(pshift)) == np.uint32(prefix)]
    b = (u >> np.uint32(shift)) & np.uint32((1 << width) - 1)
    return np.bincount(b, minlength=4096).astype(np.int64)


def top_keys_ref(d, x, m: int) -> np.ndarray:
    """Keys of the m farthest samples and the runner-up, descending (plain sort of the keys: np.lexsort on the values would
    take -0.0 and +0.0 for equal, which the keys do not)."""
    k = key64(d, x)
    return np.sort(k)[::-1][: min(m + 1, k.size)]


def ref_sums_ref(x, mean, labels, k: int):
    """(sums float32[k], counts int64[k]): per cluster the float32 running sum in sample order, from +0.0, of
    float32(x[i] - mean).  The leading +0.0 matters: without it a cluster of -0.0 terms would sum to -0.0."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    l = _unsigned(labels)
    sums = np.zeros(k, dtype=np.float32)
    counts = np.zeros(k, dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(k):
            v = (x[l == j] - np.float32(mean)).astype(np.float32)
            sums[j] = np.cumsum(np.concatenate([[np.float32(0)], v]), dtype=np.float32)[-1]
            counts[j] = v.size
    return sums, counts


def levels_ref(d, m: int, cap: int = TOPM_CAP):
    """The level logic of the farthest-sample selection, emulated: (levels used, candidates at the end, whether the general
    selection over all keys is taken).  Per level: histogram of the next value bits inside the prefix found so far, the highest
    bin that still leaves min(m + 1, n) samples at or above it, and a stop once at most ``cap`` candidates are left."""
    n = np.asarray(d).size
    need = min(m + 1, n)
    prefix, decided, cand, used = None, 0, n, 0
    for shift, width, pshift in TOPM_LEVELS:
        h = topm_hist_ref(d, shift, width, pshift, 0 if prefix is None else prefix)
        above = np.cumsum(h[::-1])[::-1] + decided
        ok = np.nonzero(above >= need)[0]
        b = int(ok[-1]) if ok.size else 0
        cand = int(above[b])
        decided = int(above[b + 1]) if b + 1 < above.size else decided
        prefix = b if prefix is None else ((prefix << width) | b)
        used += 1
        if cand <= cap:
            break
    return used, cand, cand > cap


# --------------------------------------------------------------------------------------------------------------------- case data
SELECTION_N = 200_000
SELECTION_M = (1, 7, 150)
# (levels used, fallback) per distribution and m, as levels_ref finds them (tests/test_blocks_ref.py checks the claim)
SELECTION_STOPS = {
    "tail": {1: (1, False), 7: (1, False), 150: (1, False)},
    "one_bin": {1: (2, False), 7: (2, False), 150: (2, False)},
    "one_prefix": {1: (3, False), 7: (3, False), 150: (3, False)},
    "crowd": {1: (1, False), 7: (3, True), 150: (3, True)},
}


def selection_distances(n: int = SELECTION_N, seed: int = 11) -> dict:
    """Four non-negative distance vectors, one per way the selection can end.
    tail: a sparse upper tail, the first 12 bits decide.  one_bin: 1 + rand * 0.124, which crowds the first-level bin at the cut
    far beyond the cap (the values share the exponent and three mantissa bits; they fill at most two 12-bit bins).
    one_prefix: 128 adjacent floats that share one 24-bit prefix, so only the last 7 bits tell them apart.  crowd: one value
    everywhere but at 5 seeded positions, more than the cap of exactly equal distances at the cut."""
    rng = np.random.RandomState(seed)
    out = {}
    out["tail"] = (rng.standard_normal(n).astype(np.float32) ** 2) * np.float32(1e-4)
    out["one_bin"] = (1.0 + rng.rand(n) * 0.124).astype(np.float32)
    out["one_prefix"] = from_bits(np.uint32(QUARTER_BITS) + rng.randint(0, 128, size=n).astype(np.uint32))
    crowd = np.full(n, 0.25, dtype=np.float32)
    crowd[rng.choice(n, 5, replace=False)] = np.float32(0.5) + np.arange(5, dtype=np.float32)
    out["crowd"] = crowd
    return out


def selection_values(n: int = SELECTION_N, seed: int = 12) -> np.ndarray:
    """Sample values for the keys: few distinct values (duplicates), negatives and both zeros."""
    rng = np.random.RandomState(seed)
    x = (np.round(rng.standard_normal(n) * 8) / 8).astype(np.float32)     # rounding a small negative gives -0.0
    assert np.any(bits(x) == 0x80000000) and np.any(bits(x) == 0) and np.any(x < 0)
    return x


def linspace32(lo, hi, wide: bool = False) -> np.ndarray:
    """The 32 steps of get_weight_distribution, in float32 arithmetic as the pipeline takes them; ``wide``: computed in float64
    and rounded, for a range whose width overflows float32 (+-FLT_MAX)."""
    if wide:
        return np.linspace(float(lo), float(hi), 32).astype(np.float32)
    return np.linspace(np.float32(lo), np.float32(hi), 32).astype(np.float32)


def hist_cases(seed: int = 21) -> dict:
    """name -> (x, steps32, skip_zeros) for the histogram and the ranks."""
    rng = np.random.RandomState(seed)
    cases = {}
    # (a) special values, steps over their own range: with +-FLT_MAX (everything ordinary in the two middle bins) and without
    for name, huge in (("a_special_huge", True), ("a_special", False)):
        x = special_f32(70_001, seed + (1 if huge else 2), huge=huge)
        cases[name] = (x, linspace32(x.min(), x.max(), wide=huge), False)
    # (b) every one of the 32 steps several times, among values in between
    steps = linspace32(-0.31, 0.33)
    x = np.concatenate([np.repeat(steps, 3), rng.uniform(-0.31, 0.33, 1000).astype(np.float32)])
    cases["b_on_every_step"] = (rng.permutation(x), steps, False)
    # (c) a narrow range: 6 adjacent float32 values, 10 copies each -> the steps repeat
    six = from_bits(bits(np.float32(1.0))[0] + np.arange(6, dtype=np.uint32))
    x = rng.permutation(np.repeat(six, 10))
    cases["c_repeated_steps"] = (x, linspace32(x.min(), x.max()), False)
    # (d) a constant vector: 32 equal steps, every bin empty
    x = np.full(1025, 0.375, dtype=np.float32)
    cases["d_constant"] = (x, linspace32(0.375, 0.375), False)
    # (e) both zeros strictly inside a bin, counted or skipped
    x = special_f32(8193, seed + 3, huge=False)
    steps = linspace32(x.min(), x.max())
    cases["e_zeros_counted"] = (x, steps, False)
    cases["e_zeros_skipped"] = (x, steps, True)
    # (f) values below steps[0] and above steps[31], NaN and +-inf: no bin
    x = special_f32(8191, seed + 4, huge=True, inf=True, nan=True)
    cases["f_outside"] = (x, linspace32(-0.05, 0.05), False)
    return cases


def rank_edge_values(xs) -> np.ndarray:
    """Values whose rank in the ascending xs is decided at an edge: below all, above all, +-inf, both zeros, the two ends, and
    members of runs of duplicates with their float32 neighbours."""
    xs = np.ascontiguousarray(xs, dtype=np.float32)
    dup = xs[1:][xs[1:] == xs[:-1]]
    with np.errstate(over="ignore"):        # the neighbour of +-FLT_MAX is +-inf
        head = [np.nextafter(xs[0], np.float32(-np.inf)), np.nextafter(xs[-1], np.float32(np.inf)), -np.inf, np.inf, -0.0, 0.0,
                xs[0], xs[-1]]
        if dup.size:
            for v in (dup[0], dup[dup.size // 2], dup[-1]):
                head += [v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))]
    return np.array(head, dtype=np.float32)


def rank_values(xs, m: int, seed: int = 31) -> np.ndarray:
    """m values to rank: the edge values first (as many as fit), then random members of xs and values in between, shuffled."""
    rng = np.random.RandomState(seed + m)
    xs = np.ascontiguousarray(xs, dtype=np.float32)
    fin = xs[np.isfinite(xs)] if np.isfinite(xs).any() else np.zeros(1, dtype=np.float32)
    rest = np.concatenate([rng.choice(xs, m), rng.uniform(fin[0], fin[-1], m).astype(np.float32)]).astype(np.float32)
    return rng.permutation(np.concatenate([rank_edge_values(xs), rng.permutation(rest)])[:m])


def labels_with_outliers(n: int, k: int, label_bytes: int, seed: int) -> np.ndarray:
    """Unsigned labels (uint8 / uint16): mostly indices < k, about one in eight >= k up to the largest the type holds (none
    when k fills the type), with the first index out of range and the largest one present when there is room."""
    rng = np.random.RandomState(seed)
    dt, top = (np.uint8, 255) if label_bytes == 1 else (np.uint16, 65535)
    l = rng.randint(0, k, size=n).astype(dt)
    if k <= top:
        out = rng.rand(n) < 0.125
        l[out] = rng.randint(k, top + 1, size=int(out.sum())).astype(dt)
        if n >= 2:
            p = rng.choice(n, 2, replace=False)
            l[p[0]], l[p[1]] = k, top
        else:
            l[0] = top
    return l


def ref_sums_case(n: int, k: int, label_bytes: int, seed: int):
    """(x, labels) for the sequential M-step sums: the odd clusters have no member, cluster 0 holds only -0.0 values, cluster 2
    (if there is one) the terms 1e8, 1, -1e8, 1, ... in sample order (the order decides the float32 result), the other even
    clusters bell-shaped values; one label in eight is >= k."""
    rng = np.random.RandomState(seed)
    dt, top = (np.uint8, 255) if label_bytes == 1 else (np.uint16, 65535)
    even = np.arange(0, k, 2)
    l = rng.choice(even, size=n).astype(dt)
    if k <= top:
        out = rng.rand(n) < 0.125
        l[out] = rng.randint(k, top + 1, size=int(out.sum())).astype(dt)
    x = (rng.standard_normal(n) * 0.05).astype(np.float32)
    x[l == 0] = np.float32(-0.0)
    m2 = np.nonzero(l == 2)[0]
    x[m2] = np.array([1e8, 1.0, -1e8, 1.0], dtype=np.float32)[np.arange(m2.size) % 4]
    return x, l
