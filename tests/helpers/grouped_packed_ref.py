"""The case list of the group-wise packed codebook matmul tests (nnc_cbpk_grouped, csrc/nnc_cbpk_grouped.hip, DESIGN.md section
18), shared by tests/test_grouped_packed_codebook_abi.py (CPU: the plan) and tests/test_gpu_grouped_packed_codebook.py.

The data and the float64 reference are those of the byte-form grouped tests (grouped_ref.exact_data / float_data / weights /
reference: group g's centres are offset by 64 g, so a row read from another group's table is off by 64 or more per unit of x),
the packed buffer is packed_ref.pack of the same labels.

- ``CASES``: (m, kdim, ncols, K, group_rows) with bits = 2 for K <= 4 and 4 otherwise: the smallest shapes at which a wave or a
  workgroup changes tables in every way it can.  x and bias are plain tensors and misaligned views, rotating as in grouped_ref.
- ``regime_of`` / ``required_regimes``: {stream, tiled} x {2, 4 bits} x {direct, split} for float32 x, the stream kernel again for
  both half types, the MFMA tile x {2, 4} x {direct, split} for both.
- ``walks_of``: per kernel "three groups in a split" and, for the stream and the tiled kernel, "a split starts inside a group"; the
  MFMA tile's splits start on multiples of 32, so its second way is "a split starts in a later group than 0".
Test infrastructure only."""
from __future__ import annotations

import itertools

from . import grouped_ref, packed_ref  # noqa: F401  (packed_ref.pack is the layout the tests pack with)
from .grouped_ref import DT_CODE, DTYPES, PATH_MFMA, PATH_STREAM, PATH_TILED, split_ranges, torch_dtype  # noqa: F401

CU_COUNTS = (1, 64, 256, 1024)


def bits_of(k: int) -> int:
    return 2 if k <= 4 else 4


def _case(m, kdim, ncols, k, group_rows, x_view=False, bias=True, bias_view=False):
    return dict(m=m, kdim=kdim, ncols=ncols, k=k, group_rows=group_rows, bits=bits_of(k), x_view=x_view, bias=bias, bias_view=bias_view)


CASES = [
    _case(16, 112, 70, 16, 32),                             # stream direct over 4 groups, a short last group
    _case(16, 112, 64, 4, 32, x_view=True),                 # the same at 2 bits
    _case(1, 112, 70, 3, 32, bias_view=True),               # stream split that starts inside a group, 2 bits
    _case(2, 112, 48, 16, 32, bias=False),                  # stream split that starts inside a group, 4 bits
    _case(16, 600, 50, 16, 64, x_view=True),                # stream split through 4 groups
    _case(8, 300, 40, 5, 32),                               # K below 2^bits, a boundary inside a row batch
    _case(17, 112, 130, 16, 32, x_view=True),               # tiled direct, MFMA direct
    _case(17, 160, 130, 3, 32, bias_view=True),             # tiled direct, MFMA split, 2 bits
    _case(17, 300, 50, 16, 32),                             # tiled: 2 splits of 150 rows, a TB_K step across row 160; MFMA: 4 splits of 96 rows
    _case(17, 300, 50, 4, 32, x_view=True),                 # the same at 2 bits
    _case(130, 300, 129, 4, 64, bias=False),                # two row tiles, two column tiles
    _case(4, 20, 50, 16, 32),                               # kdim < group_rows
    _case(17, 20, 50, 3, 32, bias_view=True),               # kdim < group_rows
    _case(16, 112, 70, 16, 128),                            # one group
    _case(17, 300, 50, 5, 320, x_view=True),                # one group, split
]


def case_id(c):
    return f"m{c['m']}-kd{c['kdim']}-n{c['ncols']}-k{c['k']}-r{c['group_rows']}"


def regime_of(c, plan, dtype):
    kernel = {PATH_STREAM: "stream", PATH_TILED: "tiled", PATH_MFMA: "mfma"}[plan["path"]]
    return (kernel, c["bits"], dtype, "split" if plan["splits"] > 1 else "direct")


def required_regimes():
    req = set(itertools.product(("stream",), (2, 4), DTYPES, ("direct", "split")))
    req |= set(itertools.product(("tiled",), (2, 4), ("f32",), ("direct", "split")))
    req |= set(itertools.product(("mfma",), (2, 4), ("bf16", "fp16"), ("direct", "split")))
    return req


def walks_of(c, plan):
    """The ways a call of this plan walks through groups (a set of strings)."""
    rows, ways = c["group_rows"], set()
    if plan["max_groups_per_split"] >= 3:
        ways.add("three groups in a split")
    if plan["splits"] > 1:
        starts = [lo for lo, _ in split_ranges(plan, c["kdim"])]
        if plan["path"] == PATH_MFMA:
            assert all(lo % 32 == 0 for lo in starts), plan
            if any(lo // rows > 0 for lo in starts):
                ways.add("a split starts in a later group than 0")
        elif any(lo % rows for lo in starts):
            ways.add("a split starts inside a group")
    return ways


def required_walks(kernel):
    return {"three groups in a split", "a split starts in a later group than 0" if kernel == "mfma" else "a split starts inside a group"}
