"""References and the case list for the bitmap-sparse form of the group-wise codebook layer (ops.pack_grouped_sparse_codes /
grouped_sparse_codebook_matmul, csrc/nnc_cbsp_grouped.hip), shared by
tests/test_grouped_sparse_codebook_abi.py (CPU: the plan) and tests/test_gpu_zero_symbols_grouped_sparse_codebook.py.

- ``pack_np``: a NumPy packer of the form with one skipped symbol per group (sparse_ref.split_packed cuts the device buffer).
- ``formula64``: y = t + sum over stored (i, o) of x * d_g[label] (+ bias, ReLU) in float64, d rounded to float32 as the form
  defines it, t = sum_g c_{z_g} * rs_g over the groups with c_{z_g} != 0; a skipped weight of a group with c_{z_g} == 0 is absent.
- ``float_bound``: section 11's float32 bound against the float64 product with the decoded W (grouped_ref.weights), the rank-1
  magnitude taken per group.  Derived, not measured: the factor 2 and the kdim + 4 are sparse_ref.float_bound's.
- ``draw_labels``: sparse_ref.labels_at_density per group, each group with its own z and density: groups entirely pruned, groups at
  density 1.0 (their z occurs nowhere), groups with z_g >= K, and a few stored labels >= K.
- ``exact_data``: small-integer x, quarter-integer centres offset by 64 g as grouped_ref.exact_data builds them, integer bias; it
  asserts that the sum of the magnitudes of every term of every output stays below 2^24 quarter-units, so every partial sum in
  any order is exact in float32.
- ``CASES`` / ``regime_of`` / ``required_regimes`` / ``features_of`` / ``required_features``: the smallest calls that between them
  hit every kernel instantiation, direct and split, and every way a workgroup meets a group boundary.
Test infrastructure only."""
from __future__ import annotations

import itertools

import numpy as np

from . import grouped_ref, sparse_ref

U = sparse_ref.U
PATH_STREAM, PATH_TILED = 1, 2
MTS = (1, 2, 4, 8, 16)
CU_COUNTS = (1, 64, 256, 1024)
TB_K = 8
Z_PAST_K = 250                                   # a skipped byte that names no centre (K < 250 in the cases that use it)
DENSITIES = (0.1, 0.3, 0.0, 1.0, 0.05)           # by group: 0.0 an entirely pruned group, 1.0 a group whose z occurs nowhere


def _case(m, kdim, ncols, k, group_rows=32, off=0, x_view=False, bias=True):
    return dict(m=m, kdim=kdim, ncols=ncols, k=k, group_rows=group_rows, off=off, x_view=x_view, bias=bias)


CASES = [
    _case(1, 112, 70, 3, off=1),                            # stream direct, MT 1: 4 groups, a short last one, labels at an odd offset
    _case(2, 200, 50, 16, x_view=True),                     # MT 2, 7 groups: a wave's batch of 64 rows is cut at every boundary
    _case(4, 130, 64, 256, group_rows=64),                  # MT 4, K = 256
    _case(8, 63, 1, 16, off=3),                             # MT 8, one column
    _case(16, 112, 130, 16, x_view=True, bias=False),       # MT 16, three segments
    _case(1, 1000, 50, 16, off=1),                          # stream split: 3 splits of 334 rows start inside groups, 11 groups each
    _case(2, 1500, 64, 3, group_rows=96, bias=False),       # MT 2 split
    _case(4, 1000, 130, 256, group_rows=64, x_view=True),   # MT 4 split, K = 256
    _case(8, 2100, 50, 16, group_rows=128, off=5),          # MT 8 split: 8 splits of 263 rows
    _case(16, 1000, 70, 16, off=1),                         # MT 16 split
    _case(17, 112, 130, 16, off=1, x_view=True),            # tiled direct
    _case(17, 300, 50, 256, off=3),                         # tiled: 2 splits of 150 rows, a TB_K step across row 160
    _case(130, 300, 129, 3, group_rows=64, bias=False),     # two row tiles, two column tiles, split
    _case(4, 20, 50, 16, off=2),                            # kdim < group_rows: one short group
    _case(17, 20, 64, 3),                                   # the same through the tiled kernel
    _case(16, 112, 70, 16, group_rows=128),                 # group_rows >= kdim: one group
    _case(17, 300, 50, 16, group_rows=320, off=1),          # one group, tiled split
    _case(3, 1000, 64, 16, group_rows=1024),                # one group, stream split
]


def case_id(c):
    return f"m{c['m']}-kd{c['kdim']}-n{c['ncols']}-k{c['k']}-r{c['group_rows']}-o{c['off']}"


def groups_of(c):
    return -(-c["kdim"] // c["group_rows"])


def split_ranges(plan, kdim):
    return [(s * plan["rps"], min(kdim, (s + 1) * plan["rps"])) for s in range(plan["splits"])]


def regime_of(plan):
    mode = "split" if plan["splits"] > 1 else "direct"
    if plan["path"] == PATH_STREAM:
        return ("stream", plan["mt"], mode)
    assert plan["path"] == PATH_TILED, plan
    return ("tiled", mode)


def required_regimes():
    return set(itertools.product(("stream",), MTS, ("direct", "split"))) | {("tiled", "direct"), ("tiled", "split")}


def features_of(c, plan):
    """What of the group walk a call exercises, from its plan."""
    kdim, rows = c["kdim"], c["group_rows"]
    kernel = "stream" if plan["path"] == PATH_STREAM else "tiled"
    out = set()
    ranges = split_ranges(plan, kdim)
    if plan["splits"] > 1:
        if any(hi > lo and (hi - 1) // rows > lo // rows for lo, hi in ranges):
            out.add((kernel, "two groups in one split"))
        if any(lo % rows for lo, _ in ranges):
            out.add((kernel, "a split starts inside a group"))
    if kernel == "tiled":
        for lo, hi in ranges:
            if any((b - lo) % TB_K for b in range((lo // rows + 1) * rows, hi, rows)):
                out.add(("tiled", "a TB_K step across a boundary"))
    if kernel == "stream" and rows == 32 and kdim > 32:
        out.add(("stream", "a 64-row batch cut at a boundary"))
    if kdim % rows and kdim > rows:
        out.add((kernel, "a short last group"))
    if kdim < rows:
        out.add((kernel, "kdim < group_rows"))
    if rows >= kdim:
        out.add((kernel, "one group"))
    return out


def required_features():
    per_kernel = ("two groups in one split", "a split starts inside a group", "a short last group", "kdim < group_rows", "one group")
    return set(itertools.product(("stream", "tiled"), per_kernel)) | {("tiled", "a TB_K step across a boundary"),
                                                                      ("stream", "a 64-row batch cut at a boundary")}


# ------------------------------------------------------------------ the data
def zero_symbols_of(c):
    """A different z per group; every fourth group (from the third) skips a byte that names no centre where K allows one."""
    g = np.arange(groups_of(c))
    zs = (1 + 2 * g) % c["k"]
    if c["k"] < Z_PAST_K:
        zs = np.where(g % 4 == 2, Z_PAST_K, zs)
    return zs.astype(np.uint8)


def group_density(c, g, ci=0):
    return DENSITIES[(g + ci) % len(DENSITIES)]


def draw_labels(c, seed, ci=0):
    """-> (labels (kdim, ncols) int64, zero_symbols uint8[G]).  Every fourth group (from the first) of a K < 256 case stores a few
    labels equal to K (they read -c_{z_g}; the byte form reads 0 for them)."""
    rng = np.random.RandomState(seed)
    kdim, ncols, k, rows = c["kdim"], c["ncols"], c["k"], c["group_rows"]
    zs = zero_symbols_of(c)
    parts = []
    for g, z in enumerate(zs):
        n = min(kdim, (g + 1) * rows) - g * rows
        lab = sparse_ref.labels_at_density(rng, n, ncols, k, group_density(c, g, ci), int(z))
        if k < 256 and g % 4 == 0:
            flat = lab.reshape(-1)
            flat[rng.randint(0, flat.size, size=min(3, flat.size))] = k
        parts.append(lab)
    return np.concatenate(parts, axis=0), zs


def _zero_some_cz(c, cen, zs):
    """c_{z_g} = 0 exactly in every third group (from the second): its skipped weights are absent."""
    for g, z in enumerate(zs):
        if g % 3 == 1 and z < c["k"]:
            cen[g, z] = 0.0
    return cen


def cz_of(cen, zs):
    cen = np.asarray(cen, dtype=np.float32)
    k = cen.shape[1]
    return np.array([cen[g, z] if z < k else np.float32(0.0) for g, z in enumerate(zs)], dtype=np.float32)


def d_tables(cen, zs, k_all):
    """d[g][s] for s < k_all: float32(c_g[s] - c_{z_g}), -c_{z_g} past K."""
    cen = np.asarray(cen, dtype=np.float32)
    cz = cz_of(cen, zs)
    d = np.repeat((np.float32(0.0) - cz)[:, None], k_all, axis=1).astype(np.float32)
    d[:, : cen.shape[1]] = cen - cz[:, None]
    return d, cz


def row_groups(kdim, group_rows):
    return np.arange(kdim) // group_rows


def keep_mask(lab, zs, group_rows):
    lab = np.asarray(lab)
    return lab != np.asarray(zs, dtype=np.int64)[row_groups(lab.shape[0], group_rows)][:, None]


def _magnitude(x, lab, cen, zs, group_rows, bias):
    """sum_g |c_{z_g}| sum_{i in g} |x| + |x| @ |D| (+ |bias|): the sum of the magnitudes of every term of every output."""
    ax = np.abs(np.asarray(x, dtype=np.float64))
    lab = np.asarray(lab)
    kdim = lab.shape[0]
    d, cz = d_tables(cen, zs, max(int(lab.max(initial=0)) + 1, np.shape(cen)[1]))
    rg = row_groups(kdim, group_rows)
    dmag = np.where(keep_mask(lab, zs, group_rows), np.abs(d[rg[:, None], lab].astype(np.float64)), 0.0)
    mag = ax @ dmag + (ax * np.abs(cz.astype(np.float64))[rg][None, :]).sum(axis=1, keepdims=True)
    if bias is not None:
        mag = mag + np.abs(np.asarray(bias, dtype=np.float64))
    return mag


def exact_data(c, seed, ci=0):
    """-> labels, zero_symbols, x, centres, bias (or None), every sum exact in float32: x integers of magnitude <= 4 (2 or 1 where
    4 would pass the bound below), centres quarter-integers offset by 64 g, bias integers.  Asserts the bound: the magnitudes of
    all terms of an output sum to less than 2^24 quarter-units, so no partial sum in any order is rounded."""
    lab, zs = draw_labels(c, seed, ci)
    rng = np.random.RandomState(seed + 7)
    g = groups_of(c)
    cen = (rng.randint(-16, 17, size=(g, c["k"])) / 4.0 + 64.0 * np.arange(g)[:, None]).astype(np.float32)
    cen = _zero_some_cz(c, cen, zs)
    bias = rng.randint(-50, 51, size=c["ncols"]).astype(np.float32) if c["bias"] else None
    base = rng.randint(-4, 5, size=(c["m"], c["kdim"]))
    for xmax in (4, 2, 1):
        x = np.clip(base, -xmax, xmax).astype(np.float32)
        if 4.0 * _magnitude(x, lab, cen, zs, c["group_rows"], bias).max() < 2.0 ** 24:
            break
    quarter_units = 4.0 * _magnitude(x, lab, cen, zs, c["group_rows"], bias).max()
    assert quarter_units < 2.0 ** 24, (case_id(c), quarter_units)
    assert np.array_equal(cen * 4, np.round(cen * 4)) and np.array_equal(x, np.round(x))
    return lab, zs, x, cen, bias


def float_data(c, zs, seed):
    rng = np.random.RandomState(seed + 1)
    g = groups_of(c)
    x = rng.standard_normal((c["m"], c["kdim"])).astype(np.float32)
    cen = (rng.standard_normal((g, c["k"])) + 64.0 * np.arange(g)[:, None]).astype(np.float32)
    cen = _zero_some_cz(c, cen, zs)
    bias = rng.standard_normal(c["ncols"]).astype(np.float32) if c["bias"] else None
    return x, cen, bias


# ------------------------------------------------------------------ the form
def pack_np(lab, kdim, ncols, group_rows, zs):
    """-> dict(bitmap uint64[kdim, S], counts int64[kdim, S] (exclusive, row-major), symbols, nnz), as sparse_ref.pack_np with the
    bit rule labels[i, o] != zs[i // group_rows]."""
    lab = np.asarray(lab).reshape(kdim, ncols)
    segs = -(-ncols // 64)
    kept = keep_mask(lab, zs, group_rows) if kdim else np.zeros((0, ncols), dtype=bool)
    keep = np.zeros((kdim, segs * 64), dtype=bool)
    keep[:, :ncols] = kept
    k3 = keep.reshape(kdim, segs, 64).astype(np.uint64)
    bitmap = (k3 << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64) if segs else np.zeros((kdim, 0), np.uint64)
    per = keep.reshape(kdim, segs, 64).sum(axis=2).astype(np.int64).ravel()
    counts = (np.cumsum(per) - per).reshape(kdim, segs)
    return dict(bitmap=bitmap, counts=counts, symbols=lab[kept], nnz=int(kept.sum()))


# ------------------------------------------------------------------ the arithmetic
def formula64(x, lab, cen, zs, group_rows, bias=None, relu=False):
    """The defining formula in float64, row by row of W (no BLAS: NaN and Inf as they arise)."""
    x64 = np.asarray(x, dtype=np.float64)
    lab = np.asarray(lab)
    kdim, ncols = lab.shape
    d, cz = d_tables(cen, zs, max(int(lab.max(initial=0)) + 1, np.shape(cen)[1]))
    kept = keep_mask(lab, zs, group_rows)
    rg = row_groups(kdim, group_rows)
    acc = np.zeros((x64.shape[0], ncols), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(kdim):
            keep = kept[i]
            if keep.any():
                acc[:, keep] += x64[:, i: i + 1] * d[rg[i], lab[i, keep]].astype(np.float64)
        t, any_term = np.zeros((x64.shape[0], 1), dtype=np.float64), False
        for g, c in enumerate(cz):
            if c != 0:   # a NaN centre counts
                term = float(c) * x64[:, g * group_rows: (g + 1) * group_rows].sum(axis=1, keepdims=True)
                t, any_term = (t + term if any_term else term), True
        if any_term:
            acc = t + acc
        if bias is not None:
            acc = acc + np.asarray(bias, dtype=np.float64)
        if relu:
            acc = np.where(acc < 0, 0.0, acc)
    return acc


def float_bound(x, lab, cen, zs, group_rows, bias=None):
    """The float64 product with the decoded W and section 11's bound of |y - it| with the rank-1 magnitude per group:
    2 (kdim + 4) u (|x| @ |D| + sum_g |c_{z_g}| sum_{i in g} |x| + |b|) + u (|x| @ |C - c_z|)."""
    lab = np.asarray(lab)
    kdim, ncols = lab.shape
    cen = np.asarray(cen, dtype=np.float32)
    w = grouped_ref.weights(cen, lab, kdim, ncols, group_rows).astype(np.float64)
    ref = np.asarray(x, dtype=np.float64) @ w
    if bias is not None:
        ref = ref + np.asarray(bias, dtype=np.float64)
    cz = cz_of(cen, zs).astype(np.float64)
    exact_d = np.where(keep_mask(lab, zs, group_rows), np.abs(w - cz[row_groups(kdim, group_rows)][:, None]), 0.0)
    mag = _magnitude(x, lab, cen, zs, group_rows, bias)
    return ref, 2.0 * (kdim + 4) * U * mag + U * (np.abs(np.asarray(x, dtype=np.float64)) @ exact_d) + 1e-30
