"""References and the case list for the backward pass of the group-wise codebook layer from the bitmap-sparse form
(ops.grouped_sparse_codebook_matmul_dx / grouped_sparse_codebook_centroid_grad / grouped_sparse_codebook_linear,
csrc/nnc_cbspgrad_grouped.hip), shared by tests/test_grouped_sparse_codebook_grad_abi.py (CPU: the plans) and
tests/test_gpu_zero_symbols_grouped_sparse_codebook_train.py.

- The data helpers are grouped_sparse_ref's: ``draw_labels`` (a different z per group, groups entirely pruned, groups at density 1.0,
  z_q >= K, stored labels >= K), ``zero_symbols_of``, ``pack_np``, and centres built as its exact_data / float_data build them
  (quarter-integers offset by 64 q; c_{z_q} == 0 exactly in every third group).
- ``dx64``: the defining formula in float64, c_{z_q} * sum_o g + the stored weights' g * d_q[label], the rank-1 term dropped per
  group where c_{z_q} == 0.
- ``dx_bound``: DESIGN.md section 13's bound taken per column's group, against g @ W^T with the decoded W in float64:
  2 (ncols + 4) u (|g| |D_q|^T + |c_{z_q}| sum_o |g|) + u (|g| |C_q - c_{z_q}|^T).  Derived, not measured.
- ``exact_data``: small-integer g and x; asserts that the magnitudes of the terms of every dx output sum to less than 2^24
  quarter-units, so every partial sum in any order (the byte form's too: |W| <= |d| + |c_z|) is exact in float32.
- ``CASES`` / ``EMPTY`` / ``regimes_of`` / ``features_of`` / ``required_*``: the smallest calls that between them reach every kernel
  instantiation, direct and split, and every way a workgroup or a tile meets a group boundary, read off the plans.
Test infrastructure only."""
from __future__ import annotations

import itertools

import numpy as np

from . import grouped_ref
from . import grouped_sparse_ref as fwd

U = 2.0 ** -24
PATH_NONE, PATH_STREAM, PATH_TILED, PATH_ZERO = 0, 1, 2, 4
MTS = (1, 2, 4, 8, 16)
CU_COUNTS = (1, 64, 256, 1024)
WAVES = 4


def _case(m, kdim, ncols, k, group_rows=32, off=0, pruned=False):
    return dict(m=m, kdim=kdim, ncols=ncols, k=k, group_rows=group_rows, off=off, pruned=pruned)


CASES = [
    # m <= 16, one column block
    _case(1, 112, 70, 3, off=1),                    # MT 1: workgroups of 28 rows start inside groups; a short last group; odd offset
    _case(2, 200, 50, 16),                          # MT 2: workgroups of 29 rows; rows 29..31 are a stretch of 3: a wave has no share
    _case(4, 130, 64, 256, group_rows=64),          # MT 4, K = 256
    _case(8, 63, 1, 16, off=3),                     # MT 8, one column: batches of 16 rows cut to a wave's 8
    _case(16, 300, 65, 16),                         # MT 16, one column block of 128: batches of 32 rows cut at every boundary
    # m <= 16, several column blocks (dx: the partials and the reduce)
    _case(1, 100, 520, 16, off=1),                  # MT 1: 9 segments, the second block holds one
    _case(2, 70, 1030, 3),                          # MT 2: three column blocks
    _case(4, 96, 600, 256, group_rows=64),          # MT 4
    _case(8, 150, 260, 16, group_rows=96, off=5),   # MT 8: 5 segments in blocks of 4
    _case(16, 112, 130, 16),                        # MT 16: 3 segments in blocks of 2
    # m > 16
    _case(17, 300, 50, 256, off=3),                 # tiled direct: tiles in 4 groups, the last in 2, a short last group
    _case(17, 300, 260, 16, group_rows=64),         # dx: 2 splits of ncols; tiles in 2 groups
    _case(130, 200, 129, 3, group_rows=96),         # two tiles of m, two of ncols; tiles in 2 groups of 96
    _case(260, 140, 65, 16, group_rows=128),        # dc: 2 splits of m; tiles in 1 group, a short last group
    _case(260, 100, 50, 16),                        # dc: 2 splits of m with 4 sets of bins
    # one group
    _case(4, 20, 50, 16, off=2),                    # kdim < group_rows, stream
    _case(17, 20, 64, 3),                           # the same through the tiled kernels
    _case(16, 112, 70, 16, group_rows=128),         # group_rows >= kdim, stream
    _case(17, 300, 50, 16, group_rows=320, off=1),  # group_rows >= kdim, tiled
    # nnz = 0: every position skipped
    _case(3, 40, 50, 16, pruned=True),
    _case(17, 40, 50, 16, pruned=True),
]

# (m, kdim, ncols): dx NONE (m or kdim 0) / ZERO (ncols 0), dc ZERO
EMPTY = [(0, 50, 60), (4, 0, 60), (4, 50, 0), (20, 50, 0)]


def case_id(c):
    return fwd.case_id(c) + ("-pruned" if c["pruned"] else "")


IDS = [case_id(c) for c in CASES]
groups_of = fwd.groups_of


# ------------------------------------------------------------------ the regimes and the walks, from the plans
def regimes_of(dx_plan, dc_plan):
    out = set()
    if dx_plan["path"] == PATH_STREAM:
        out.add(("dx", "stream", dx_plan["mt"], "several blocks" if dx_plan["splits"] > 1 else "one block"))
    elif dx_plan["path"] == PATH_TILED:
        out.add(("dx", "tiled", "split" if dx_plan["splits"] > 1 else "direct"))
    else:
        out.add(("dx", {PATH_NONE: "none", PATH_ZERO: "zero"}[dx_plan["path"]]))
    if dc_plan["path"] == PATH_STREAM:
        out.add(("dc", "stream", dc_plan["mt"]))
    elif dc_plan["path"] == PATH_TILED:
        out.add(("dc", "tiled", "split" if dc_plan["splits"] > 1 else "direct"))
    else:
        assert dc_plan["path"] == PATH_ZERO
        out.add(("dc", "zero"))
    return out


def required_regimes():
    req = {("dx", "stream", mt, b) for mt, b in itertools.product(MTS, ("one block", "several blocks"))}
    req |= {("dx", "tiled", "direct"), ("dx", "tiled", "split"), ("dx", "none"), ("dx", "zero")}
    req |= {("dc", "stream", mt) for mt in MTS} | {("dc", "tiled", "direct"), ("dc", "tiled", "split"), ("dc", "zero")}
    return req


def stretches(plan, kdim, rows):
    """Per stream workgroup: (s_lo, s_hi, [(lo, hi) of every stretch]) as the kernels walk them."""
    rpg = plan["rows_per_group"]
    out = []
    for w in range(plan["row_tiles"]):
        s_lo, s_hi = w * rpg, min(kdim, (w + 1) * rpg)
        st, lo = [], s_lo
        while lo < s_hi:
            hi = min(s_hi, (lo // rows + 1) * rows)
            st.append((lo, hi))
            lo = hi
        out.append((s_lo, s_hi, st))
    return out


def wave_shares(lo, hi):
    per = -(-(hi - lo) // WAVES)
    starts = [min(hi, lo + w * per) for w in range(WAVES)]
    return [(i0, min(hi, i0 + per)) for i0 in starts]


def features_of(c, which, plan):
    """What of the group walk the ``which`` ("dx" / "dc") call of a case exercises, from its plan."""
    kdim, rows = c["kdim"], c["group_rows"]
    out = set()
    if plan["path"] == PATH_STREAM:
        kern = (which, "stream")
        rb = 64 // plan["segs"]
        for s_lo, s_hi, st in stretches(plan, kdim, rows):
            assert s_hi > s_lo and st[0][0] == s_lo and st[-1][1] == s_hi and len(st) <= plan["max_groups_per_workgroup"]
            if len(st) >= 2:
                out.add(kern + ("a workgroup in two groups or more",))
            if s_lo % rows:
                out.add(kern + ("a workgroup starts inside a group",))
            for lo, hi in st:
                shares = wave_shares(lo, hi)
                if any(i1 == i0 for i0, i1 in shares):
                    out.add(kern + ("a wave with an empty share",))
                if rows == 32 and any((i1 - i0) % rb for i0, i1 in shares):
                    out.add(kern + ("a batch cut at a boundary",))
    elif plan["path"] == PATH_TILED:
        kern = (which, "tiled")
        for t0 in range(0, kdim, 128):
            span = (min(kdim, t0 + 128) - 1) // rows - t0 // rows + 1
            assert span <= plan["max_groups_per_workgroup"]
            if rows < kdim:
                out.add(kern + (f"a tile in {span} groups",))
    else:
        return out
    if kdim % rows and kdim > rows:
        out.add(kern + ("a short last group",))
    if kdim < rows:
        out.add(kern + ("kdim < group_rows",))
    if rows >= kdim:
        out.add(kern + ("one group",))
    return out


def required_features():
    stream = ("a workgroup in two groups or more", "a workgroup starts inside a group", "a wave with an empty share", "a batch cut at a boundary",
              "a short last group", "kdim < group_rows", "one group")
    tiled = ("a tile in 4 groups", "a tile in 2 groups", "a tile in 1 groups", "a short last group", "one group")
    return {(w, "stream", f) for w in ("dx", "dc") for f in stream} | {(w, "tiled", f) for w in ("dx", "dc") for f in tiled}


# ------------------------------------------------------------------ the data
def labels_of(c, seed, ci=0):
    """-> (labels (kdim, ncols) int64, zero_symbols uint8[G]): grouped_sparse_ref.draw_labels, or every position the group's z."""
    if not c["pruned"]:
        return fwd.draw_labels(c, seed, ci)
    zs = fwd.zero_symbols_of(c)
    return np.repeat(zs.astype(np.int64)[fwd.row_groups(c["kdim"], c["group_rows"])][:, None], c["ncols"], axis=1), zs


def _dx_magnitude(g, lab, cen, zs, rows):
    """|c_{z_q}| sum_o |g| + |g| @ |D_q|^T: the sum of the magnitudes of every term of every dx output."""
    ag = np.abs(np.asarray(g, dtype=np.float64))
    lab = np.asarray(lab)
    d, cz = fwd.d_tables(cen, zs, max(int(lab.max(initial=0)) + 1, np.shape(cen)[1]))
    rg = fwd.row_groups(lab.shape[0], rows)
    dmag = np.where(fwd.keep_mask(lab, zs, rows), np.abs(d[rg[:, None], lab].astype(np.float64)), 0.0)
    return ag @ dmag.T + ag.sum(axis=1, keepdims=True) * np.abs(cz.astype(np.float64))[rg][None, :]


def exact_data(c, seed, ci=0):
    """-> labels, zero_symbols, x, g, centres, every dx sum exact in float32: g integers of magnitude <= 4 (2 or 1 where 4 would
    pass the bound), x integers in [-3, 3], centres quarter-integers offset by 64 q.  Asserts the bound."""
    lab, zs = labels_of(c, seed, ci)
    rng = np.random.RandomState(seed + 7)
    G = groups_of(c)
    cen = (rng.randint(-16, 17, size=(G, c["k"])) / 4.0 + 64.0 * np.arange(G)[:, None]).astype(np.float32)
    cen = fwd._zero_some_cz(c, cen, zs)
    x = rng.randint(-3, 4, size=(c["m"], c["kdim"])).astype(np.float32)
    base = rng.randint(-4, 5, size=(c["m"], c["ncols"]))
    for gmax in (4, 2, 1):
        g = np.clip(base, -gmax, gmax).astype(np.float32)
        if 4.0 * _dx_magnitude(g, lab, cen, zs, c["group_rows"]).max(initial=0.0) < 2.0 ** 24:
            break
    quarter_units = 4.0 * _dx_magnitude(g, lab, cen, zs, c["group_rows"]).max(initial=0.0)
    assert quarter_units < 2.0 ** 24, (case_id(c), quarter_units)
    assert np.array_equal(cen * 4, np.round(cen * 4)) and np.array_equal(g, np.round(g))
    return lab, zs, x, g, cen


def float_data(c, zs, seed):
    rng = np.random.RandomState(seed + 1)
    G = groups_of(c)
    x = rng.standard_normal((c["m"], c["kdim"])).astype(np.float32)
    g = rng.standard_normal((c["m"], c["ncols"])).astype(np.float32)
    cen = (rng.standard_normal((G, c["k"])) + 64.0 * np.arange(G)[:, None]).astype(np.float32)
    return x, g, fwd._zero_some_cz(c, cen, zs)


# ------------------------------------------------------------------ the arithmetic
def dx64(g, lab, cen, zs, rows):
    """The defining formula in float64, column by column of dx (no BLAS: NaN and Inf as they arise)."""
    g64 = np.asarray(g, dtype=np.float64)
    lab = np.asarray(lab)
    kdim = lab.shape[0]
    d, cz = fwd.d_tables(cen, zs, max(int(lab.max(initial=0)) + 1, np.shape(cen)[1]))
    kept = fwd.keep_mask(lab, zs, rows)
    rg = fwd.row_groups(kdim, rows)
    out = np.zeros((g64.shape[0], kdim), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        rs = g64.sum(axis=1)
        for i in range(kdim):
            keep = kept[i]
            acc = (g64[:, keep] * d[rg[i], lab[i, keep]].astype(np.float64)[None, :]).sum(axis=1) if keep.any() else np.zeros(g64.shape[0])
            c = cz[rg[i]]
            out[:, i] = float(c) * rs + acc if c != 0 else acc   # a NaN centre counts
    return out


def dx_bound(g, lab, cen, zs, rows):
    """(g @ W^T in float64 with the decoded W, the bound of |dx - it| per element)."""
    lab = np.asarray(lab)
    kdim, ncols = lab.shape
    cen = np.asarray(cen, dtype=np.float32)
    w = grouped_ref.weights(cen, lab, kdim, ncols, rows).astype(np.float64)
    g64 = np.asarray(g, dtype=np.float64)
    cz = fwd.cz_of(cen, zs).astype(np.float64)
    exact_d = np.where(fwd.keep_mask(lab, zs, rows), np.abs(w - cz[fwd.row_groups(kdim, rows)][:, None]), 0.0)
    return g64 @ w.T, 2.0 * (ncols + 4) * U * _dx_magnitude(g, lab, cen, zs, rows) + U * (np.abs(g64) @ exact_d.T) + 1e-30
