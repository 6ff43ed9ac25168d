"""The case list and the float64 references of the group-wise codebook backward tests (nnc_cbmm_grouped_dx_f32 /
nnc_cbmm_grouped_dc_f32, csrc/nnc_cbgrad_grouped.hip), shared by tests/test_grouped_codebook_grad_abi.py
(CPU: the plans) and tests/test_gpu_grouped_codebook_backward.py.

- ``CASES``: (m, kdim, ncols, K, group_rows, label offset), the smallest shapes at which each walk can go wrong, worked out from
  the ungrouped plans at 256 CUs; ``EXPECT`` holds what each comment claims as plan fields, which the ABI test asserts.
- ``exact_data`` / ``float_data``: group q's centres are offset by 64 q (as grouped_ref), so a row read from the wrong table shows.
- ``dx64`` / ``dc64`` and ``dx_bound`` / ``dc_bound``: cbgrad_ref's formulas and bounds, taken group by group.
- ``labels16``: the one-codebook image of the grouped indices, q * K + label, for the identity with codebook_centroid_grad.
- ``exact_data`` / ``labels_of`` and the formulas also serve tests/helpers/stream_cells_ref.py, whose cases reach every stream instantiation
  (DESIGN.md section 29).
Test infrastructure only."""
from __future__ import annotations

import numpy as np

from . import cbgrad_ref, grouped_ref

PATH_NONE, PATH_STREAM, PATH_TILED, PATH_ZERO = cbgrad_ref.PATH_NONE, cbgrad_ref.PATH_STREAM, cbgrad_ref.PATH_TILED, cbgrad_ref.PATH_ZERO
CU_COUNTS = grouped_ref.CU_COUNTS


def _case(m, kdim, ncols, k, group_rows, off=0):
    return dict(m=m, kdim=kdim, ncols=ncols, k=k, group_rows=group_rows, off=off)


STREAM_CASES = [
    _case(16, 112, 70, 16, 32, 1),      # 4 row groups of 28 rows: workgroups start inside groups, boundaries inside a wave's 7 rows, a short last group, unaligned rows
    _case(8, 93, 40, 256, 32),          # row groups of 31: the second workgroup's first wave takes a batch of 8 rows across row 32; K = 256
    _case(1, 300, 2500, 3, 32, 3),      # three column blocks: the dx partials go through the reduce; unaligned rows
    _case(2, 112, 48, 16, 32),          # aligned rows
    _case(16, 200, 32768, 16, 32),      # 128 column blocks, so four row groups of 50 rows: one workgroup walks three groups (the one large case)
]
TILED_CASES = [
    _case(17, 112, 130, 16, 32, 1),     # one dx tile over four groups; two dc column tiles
    _case(17, 300, 300, 256, 96),       # dx tiles over groups {0,1}, {1,2}, {2,3}; ncols split in two; K = 256
    _case(300, 160, 129, 3, 64),        # the dc reduction over m split in two; three dx row tiles
]
ONE_GROUP_CASES = [_case(16, 112, 70, 16, 128), _case(17, 300, 50, 256, 320, 1)]
SHORT_CASES = [_case(4, 20, 50, 16, 32), _case(17, 20, 50, 3, 32)]             # kdim < group_rows
EMPTY_CASES = [_case(0, 50, 60, 8, 32), _case(4, 0, 60, 8, 32), _case(20, 0, 60, 8, 32), _case(4, 50, 0, 8, 32), _case(20, 50, 0, 8, 32)]
CASES = STREAM_CASES + TILED_CASES + ONE_GROUP_CASES + SHORT_CASES
ALL_CASES = CASES + EMPTY_CASES


def case_id(c):
    return f"m{c['m']}-kd{c['kdim']}-n{c['ncols']}-k{c['k']}-r{c['group_rows']}-o{c['off']}"


# what the comments above claim, as fields of the plans at 256 CUs (dx: / dc: prefixes) -- asserted by the ABI test
EXPECT = {
    case_id(STREAM_CASES[0]): {"dx:path": PATH_STREAM, "dx:rows_per_group": 28, "dx:row_tiles": 4, "dx:aligned": 0, "dx:groups": 4,
                               "dx:max_groups_per_workgroup": 2, "dc:path": PATH_STREAM, "dc:rows_per_group": 28},
    case_id(STREAM_CASES[1]): {"dx:path": PATH_STREAM, "dx:rows_per_group": 31, "dx:row_tiles": 3, "dx:mt": 8, "dc:rows_per_group": 31},
    case_id(STREAM_CASES[2]): {"dx:path": PATH_STREAM, "dx:col_tiles": 3, "dx:splits": 3, "dx:aligned": 0},
    case_id(STREAM_CASES[3]): {"dx:path": PATH_STREAM, "dx:aligned": 1, "dc:aligned": 1},
    case_id(STREAM_CASES[4]): {"dx:path": PATH_STREAM, "dx:col_tiles": 128, "dx:row_tiles": 4, "dx:rows_per_group": 50,
                               "dx:max_groups_per_workgroup": 3, "dc:max_groups_per_workgroup": 3},
    case_id(TILED_CASES[0]): {"dx:path": PATH_TILED, "dx:col_tiles": 1, "dx:max_groups_per_workgroup": 4, "dx:copies": 4, "dc:path": PATH_TILED,
                              "dc:col_tiles": 2, "dc:max_groups_per_workgroup": 4},
    case_id(TILED_CASES[1]): {"dx:path": PATH_TILED, "dx:col_tiles": 3, "dx:splits": 2, "dx:max_groups_per_workgroup": 2, "dx:groups": 4},
    case_id(TILED_CASES[2]): {"dx:path": PATH_TILED, "dx:row_tiles": 3, "dc:path": PATH_TILED, "dc:splits": 2},
    case_id(ONE_GROUP_CASES[0]): {"dx:path": PATH_STREAM, "dx:groups": 1, "dx:max_groups_per_workgroup": 1},
    case_id(ONE_GROUP_CASES[1]): {"dx:path": PATH_TILED, "dx:groups": 1, "dc:max_groups_per_workgroup": 1},
    case_id(SHORT_CASES[0]): {"dx:path": PATH_STREAM, "dx:groups": 1},
    case_id(SHORT_CASES[1]): {"dx:path": PATH_TILED, "dc:path": PATH_TILED, "dx:groups": 1},
}

# the plan fields a grouped plan shares with the ungrouped one of (m, kdim, ncols, label_bytes 1, k, cus)
DX_SHARED = ("path", "vb", "mt", "splits", "cps", "aligned", "col_tiles", "row_tiles", "workspace")
DC_SHARED = ("path", "vb", "mt", "splits", "rps", "aligned", "col_tiles", "row_tiles", "terms_log2")


def groups_of(c):
    """G as the layers count it: one row of centres even where kdim = 0."""
    return max(1, -(-c["kdim"] // c["group_rows"]))


def group_rows_of(c, q):
    return slice(q * c["group_rows"], min(c["kdim"], (q + 1) * c["group_rows"]))


def max_groups(extent, per, kdim, group_rows):
    """The most groups the rows [s * per, min(kdim, (s + 1) * per)) of one workgroup lie in."""
    most = 0
    for lo in range(0, kdim, per):
        hi = min(kdim, lo + per)
        most = max(most, (hi - 1) // group_rows - lo // group_rows + 1)
    return most


def labels_of(c, seed, oob=False):
    """(kdim, ncols) indices in [0, K), or with ``oob`` up to K + 2 (at most 255)."""
    rng = np.random.RandomState(seed)
    top = min(c["k"] + 3, 256) if oob else c["k"]
    return rng.randint(0, top, size=(c["kdim"], c["ncols"]))


def exact_data(c, seed):
    """integer x and g in [-3, 3], quarter-integer centres offset by 64 q."""
    rng = np.random.RandomState(seed + 17)
    x = rng.randint(-3, 4, size=(c["m"], c["kdim"])).astype(np.float32)
    g = rng.randint(-3, 4, size=(c["m"], c["ncols"])).astype(np.float32)
    G = groups_of(c)
    cen = (rng.randint(-8, 9, size=(G, c["k"])) / 4.0 + 64.0 * np.arange(G)[:, None]).astype(np.float32)
    return x, g, cen


def float_data(c, seed):
    rng = np.random.RandomState(seed + 29)
    x = (rng.standard_normal((c["m"], c["kdim"])) * 0.7).astype(np.float32)
    g = (rng.standard_normal((c["m"], c["ncols"])) * 1e-2).astype(np.float32)
    G = groups_of(c)
    cen = (rng.standard_normal((G, c["k"])) + 64.0 * np.arange(G)[:, None]).astype(np.float32)
    return x, g, cen


def decoded(c, lab, cen):
    """W (kdim, ncols) float64, 0 for an index >= K."""
    w = np.zeros((c["kdim"], c["ncols"]))
    for q in range(groups_of(c)):
        rows = group_rows_of(c, q)
        w[rows] = cbgrad_ref.decoded(lab[rows], cen[q])
    return w


def dx64(c, g, lab, cen):
    return np.asarray(g, dtype=np.float64) @ decoded(c, lab, cen).T


def dx_bound(c, g, lab, cen):
    return 2.0 * (c["ncols"] + 4) * cbgrad_ref.U * (np.abs(np.asarray(g, dtype=np.float64)) @ np.abs(decoded(c, lab, cen)).T)


def dc64(c, x, g, lab):
    """(G, K) float64: group q's bins over its own rows."""
    out = np.zeros((groups_of(c), c["k"]))
    if c["m"] * c["kdim"] * c["ncols"] == 0:
        return out
    for q in range(groups_of(c)):
        rows = group_rows_of(c, q)
        out[q] = cbgrad_ref.dc64(x[:, rows], g, lab[rows], c["k"])
    return out


def dc_bound(c, x, g, lab, S, f32_out=False):
    out = np.zeros((groups_of(c), c["k"]))
    for q in range(groups_of(c)):
        rows = group_rows_of(c, q)
        out[q] = cbgrad_ref.dc_bound(x[:, rows], g, lab[rows], c["k"], S, f32_out=f32_out)
    return out


def labels16(c, lab):
    """q * K + label: the grouped indices as those of one codebook of G * K centres (all labels below K)."""
    return (np.arange(c["kdim"]) // c["group_rows"])[:, None] * c["k"] + lab
