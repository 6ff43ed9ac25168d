"""The case list and the references of the group-wise packed codebook backward tests (nnc_cbpk_grouped_dx_f32 /
nnc_cbpk_grouped_dc_f32, csrc/nnc_cbpkgrad_grouped.hip), shared by
tests/test_grouped_packed_codebook_grad_abi.py (CPU: the plans) and tests/test_gpu_grouped_packed_codebook_backward.py.

- ``CASES``: dicts of (m, kdim, ncols, bits, k, group_rows).  Every case of packed_grad_ref.CASES at group_rows 32 (between them
  every (bits, mt) and rows that leave padding), then crafted shapes, the smallest at which each walk can go wrong, worked out
  from the ungrouped packed plans at 256 CUs; ``EXPECT`` holds what each comment claims as plan fields, which the ABI test asserts.
- ``WIDE_CASES``: the stream instantiations with 8- and 16-byte loads are planned only where column blocks x 32-row batches fill
  the planning device, so they need 16 to 67 million indices: the plans are checked on the CPU, the identities with the existing
  ops once each on the GPU, no float64 reference is formed.
- The data and the float64 formulas are grouped_grad_ref's (group q's centres offset by 64 q, so a row read from the wrong table
  shows) on the labels the packed buffer holds (packed_grad_ref.held_labels); labels are drawn up to 2^bits - 1, so labels >= K
  occur whenever K < 2^bits.
Test infrastructure only."""
from __future__ import annotations

import numpy as np

from . import grouped_grad_ref as ggr
from . import packed_grad_ref as pgr

PATH_NONE, PATH_STREAM, PATH_TILED, PATH_ZERO = pgr.PATH_NONE, pgr.PATH_STREAM, pgr.PATH_TILED, pgr.PATH_ZERO
CU_COUNTS = (1, 8, 104, 256, 304)


def _case(m, kdim, ncols, bits, k, group_rows):
    return dict(m=m, kdim=kdim, ncols=ncols, bits=bits, k=k, group_rows=group_rows, off=0)


PACKED_CASES = [_case(m, kdim, ncols, bits, k, 32) for _, m, kdim, ncols, bits, k in pgr.CASES]
STREAM_CASES = [
    _case(16, 112, 70, 4, 16, 32),      # 4 row groups of 28 rows: workgroups start inside groups, boundaries inside a wave's 7 rows, a short last group; vb 2, mt 16
    _case(8, 93, 40, 2, 4, 32),         # 3 row groups of 31: a batch of 8 rows lies across row 32; vb 2, mt 8
    _case(1, 300, 2500, 2, 3, 32),      # 3 column blocks: dx through the reduce; K = 3 at 2 bits, so label 3 occurs; 10 row groups
    _case(1, 300, 2500, 4, 3, 32),      # K = 3 at the wider 4-bit form (labels up to 15 >= K); 5 column blocks
    _case(2, 112, 48, 4, 16, 32),       # rows that fill their 16-byte groups less one: padding fields present
    _case(2, 70, 100, 2, 4, 32),        # (bits 2, vb 4, mt 2) over three groups: packed_grad_ref has it at kdim = 1 only
    _case(16, 200, 32768, 4, 16, 32),   # 128 column blocks, so 4 row groups of 50: one workgroup walks three groups (the one large case, 6.5 M indices)
]
TILED_CASES = [
    _case(17, 112, 130, 4, 16, 32),     # one dx tile over four groups; dc: 2 column tiles, one row tile over four groups (4 sets)
    _case(17, 300, 300, 2, 4, 96),      # dx tiles over groups {0,1}, {1,2}, {2,3}; ncols split in two
    _case(17, 300, 300, 4, 16, 96),
    _case(300, 160, 129, 2, 3, 64),     # dc's reduction over m split in two; 2 sets
]
ONE_GROUP_CASES = [_case(16, 112, 70, 4, 16, 128), _case(17, 300, 50, 2, 4, 320)]
SHORT_CASES = [_case(4, 20, 50, 4, 16, 32), _case(17, 20, 50, 2, 3, 32)]             # kdim < group_rows
EMPTY_CASES = [_case(c["m"], c["kdim"], c["ncols"], bits, min(c["k"], 1 << bits), c["group_rows"]) for bits in (4, 2) for c in ggr.EMPTY_CASES]
CRAFTED_CASES = STREAM_CASES + TILED_CASES + ONE_GROUP_CASES + SHORT_CASES
CASES = [c for c in PACKED_CASES if c["m"] * c["kdim"] * c["ncols"]] + CRAFTED_CASES     # the cases that compute something
ALL_CASES = PACKED_CASES + CRAFTED_CASES + EMPTY_CASES
# (m, kdim, ncols, bits, k, group_rows): three groups, the last one short; 33 rows per workgroup, so boundaries fall inside workgroups
WIDE_CASES = [_case(1, 16400, 1024, 4, 16, 8192), _case(2, 16400, 1024, 4, 16, 8192), _case(4, 16400, 1024, 4, 16, 8192),
              _case(1, 16400, 2048, 4, 16, 8192), _case(2, 16400, 2048, 4, 16, 8192),
              _case(1, 16400, 2048, 2, 4, 8192), _case(2, 16400, 2048, 2, 4, 8192), _case(1, 16400, 4096, 2, 4, 8192)]
WIDE_EXPECT = [(4, 8, 1), (4, 8, 2), (4, 8, 4), (4, 16, 1), (4, 16, 2), (2, 8, 1), (2, 8, 2), (2, 16, 1)]   # (bits, vb, mt) of each, at every CU count

# every stream instantiation of csrc/nnc_cbpkgrad_grouped.hip (kPggCases): (bits, vb, mt)
INSTANTIATIONS = {(4, 16, 1), (4, 8, 1), (4, 4, 1), (4, 16, 2), (4, 8, 2), (4, 4, 2), (4, 8, 4), (4, 4, 4), (4, 4, 8), (4, 2, 16),
                  (2, 16, 1), (2, 8, 1), (2, 4, 1), (2, 8, 2), (2, 4, 2), (2, 4, 4), (2, 2, 8), (2, 1, 16)}


def case_id(c):
    return f"m{c['m']}-kd{c['kdim']}-n{c['ncols']}-b{c['bits']}-k{c['k']}-r{c['group_rows']}"


# what the comments above claim, as fields of the plans at 256 CUs (dx: / dc: prefixes) -- asserted by the ABI test
EXPECT = {
    case_id(STREAM_CASES[0]): {"dx:path": PATH_STREAM, "dx:rows_per_group": 28, "dx:row_tiles": 4, "dx:vb": 2, "dx:mt": 16, "dx:groups": 4,
                               "dx:max_groups_per_workgroup": 2, "dc:path": PATH_STREAM, "dc:rows_per_group": 28, "dc:vb": 2, "dc:mt": 16},
    case_id(STREAM_CASES[1]): {"dx:path": PATH_STREAM, "dx:rows_per_group": 31, "dx:row_tiles": 3, "dx:vb": 2, "dx:mt": 8, "dc:rows_per_group": 31},
    case_id(STREAM_CASES[2]): {"dx:path": PATH_STREAM, "dx:col_tiles": 3, "dx:splits": 3, "dx:row_tiles": 10, "dc:row_tiles": 10},
    case_id(STREAM_CASES[3]): {"dx:path": PATH_STREAM, "dx:col_tiles": 5, "dx:splits": 5},
    case_id(STREAM_CASES[4]): {"dx:path": PATH_STREAM, "dx:mt": 2, "dx:max_groups_per_workgroup": 2},
    case_id(STREAM_CASES[5]): {"dx:path": PATH_STREAM, "dx:vb": 4, "dx:mt": 2, "dx:groups": 3},
    case_id(STREAM_CASES[6]): {"dx:path": PATH_STREAM, "dx:col_tiles": 128, "dx:row_tiles": 4, "dx:rows_per_group": 50,
                               "dx:max_groups_per_workgroup": 3, "dc:max_groups_per_workgroup": 3},
    case_id(TILED_CASES[0]): {"dx:path": PATH_TILED, "dx:col_tiles": 1, "dx:max_groups_per_workgroup": 4, "dx:held": 4, "dc:path": PATH_TILED,
                              "dc:col_tiles": 2, "dc:row_tiles": 1, "dc:max_groups_per_workgroup": 4, "dc:held": 4},
    case_id(TILED_CASES[1]): {"dx:path": PATH_TILED, "dx:col_tiles": 3, "dx:splits": 2, "dx:max_groups_per_workgroup": 2, "dx:groups": 4, "dx:held": 2},
    case_id(TILED_CASES[2]): {"dx:path": PATH_TILED, "dx:col_tiles": 3, "dx:splits": 2, "dx:max_groups_per_workgroup": 2, "dx:groups": 4, "dx:held": 2},
    case_id(TILED_CASES[3]): {"dx:path": PATH_TILED, "dc:path": PATH_TILED, "dc:splits": 2, "dc:held": 2},
    case_id(ONE_GROUP_CASES[0]): {"dx:path": PATH_STREAM, "dx:groups": 1, "dx:max_groups_per_workgroup": 1},
    case_id(ONE_GROUP_CASES[1]): {"dx:path": PATH_TILED, "dx:groups": 1, "dc:max_groups_per_workgroup": 1},
    case_id(SHORT_CASES[0]): {"dx:path": PATH_STREAM, "dx:groups": 1},
    case_id(SHORT_CASES[1]): {"dx:path": PATH_TILED, "dc:path": PATH_TILED, "dx:groups": 1},
}

# the plan fields a grouped plan shares with the ungrouped packed one of (m, kdim, ncols, bits, k, cus)
DX_SHARED = ("path", "vb", "mt", "cols", "copies", "entries", "splits", "cps", "col_tiles", "row_tiles", "workspace")
DC_SHARED = ("path", "vb", "mt", "cols", "splits", "rps", "lds", "col_tiles", "row_tiles", "terms_log2")

groups_of, group_rows_of, max_groups = ggr.groups_of, ggr.group_rows_of, ggr.max_groups
exact_data, float_data = ggr.exact_data, ggr.float_data


def labels_of(c, seed):
    """(kdim, ncols) indices in [0, 2^bits): beyond K whenever K < 2^bits."""
    return np.random.RandomState(seed).randint(0, 1 << c["bits"], size=(c["kdim"], c["ncols"]))


def held(c, lab):
    """The labels as the packed buffer holds them (the NumPy pack and unpack of the layout)."""
    return pgr.held_labels(lab, c["bits"]) if lab.size else np.asarray(lab, dtype=np.int64)


def dx64(c, g, lab, cen):
    return ggr.dx64(c, g, held(c, lab), cen)


def dx_bound(c, g, lab, cen):
    """2 (ncols + 4) u (|g| |W|^T), on the held labels.  Derived, not measured."""
    return ggr.dx_bound(c, g, held(c, lab), cen) + 1e-30


def dc64(c, x, g, lab):
    return ggr.dc64(c, x, g, held(c, lab))


def dc_bound(c, x, g, lab, S, f32_out=False):
    return ggr.dc_bound(c, x, g, held(c, lab), S, f32_out=f32_out)
