"""The case list of the tests of the group-wise bitmap-sparse layer on bf16 / fp16 activations (ops.grouped_sparse_codebook_matmul
with half_inputs=True, csrc/nnc_cbsp_grouped_h16.hip), shared by tests/test_grouped_sparse_codebook_h16_abi.py
(CPU: the plan) and tests/test_gpu_zero_symbols_grouped_sparse_codebook_h16.py.

- ``CASES``: the m <= 16 cases of grouped_sparse_ref.CASES (the stream path follows nnc_cbsp_grouped_plan) and the m > 16 cases of
  grouped_ref.CASES (the MFMA path follows nnc_cbmm_grouped_plan's half plan), in grouped_sparse_ref's case shape, so that its
  ``draw_labels`` / ``exact_data`` / ``float_data`` serve both.  Between them they reach every regime and every walk feature below
  (asserted from the plans at 256 CUs by the CPU test and at the device's CU count by the GPU test), so none is added.
- ``regime_of`` / ``required_regimes``: {stream} x MT x {direct, split} and {mfma} x {direct, split}, each with both dtypes.
- ``features_of`` / ``required_features``: what of the group walk a call exercises, per kernel.
Test infrastructure only."""
from __future__ import annotations

import itertools

from . import grouped_ref, grouped_sparse_ref as sref, h16_ref

DTYPES = h16_ref.DTYPES
DT_CODE = h16_ref.DT_CODE
PATH_STREAM, PATH_MFMA = 1, 5
MTS = sref.MTS
CU_COUNTS = (1, 64, 256, 1024)

CASES = ([dict(c) for c in sref.CASES if c["m"] <= 16]
         + [sref._case(c["m"], c["kdim"], c["ncols"], c["k"], c["group_rows"], c["off"], c["x_view"], c["bias"]) for c in grouped_ref.CASES if c["m"] > 16])

case_id = sref.case_id
groups_of = sref.groups_of
split_ranges = sref.split_ranges


def torch_dtype(name):
    return h16_ref.torch_dtype(name)


def regime_of(plan, dtype):
    mode = "split" if plan["splits"] > 1 else "direct"
    if plan["path"] == PATH_STREAM:
        return ("stream", plan["mt"], dtype, mode)
    assert plan["path"] == PATH_MFMA, plan
    return ("mfma", dtype, mode)


def required_regimes():
    return set(itertools.product(("stream",), MTS, DTYPES, ("direct", "split"))) | set(itertools.product(("mfma",), DTYPES, ("direct", "split")))


def features_of(c, plan):
    kdim, rows = c["kdim"], c["group_rows"]
    kernel = "stream" if plan["path"] == PATH_STREAM else "mfma"
    out = set()
    ranges = split_ranges(plan, kdim)
    if any(hi > lo and (hi - 1) // rows > lo // rows for lo, hi in ranges):
        out.add((kernel, "two groups in one split"))
    if plan["splits"] > 1 and any(lo % rows for lo, _ in ranges):
        out.add((kernel, "a split starts inside a group"))
    if kdim % rows and kdim > rows:
        out.add((kernel, "a short last group"))
    if kdim < rows:
        out.add((kernel, "kdim < group_rows"))
    if rows >= kdim:
        out.add((kernel, "one group"))
    return out


def required_features():
    per_kernel = ("two groups in one split", "a split starts inside a group", "a short last group", "kdim < group_rows", "one group")
    return set(itertools.product(("stream", "mfma"), per_kernel))
