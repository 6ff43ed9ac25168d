"""The case list and the float64 reference of the group-wise codebook matmul tests (nnc_cbmm_grouped, csrc/nnc_cbmm_grouped.hip,
DESIGN.md section 17), shared by tests/test_grouped_codebook_abi.py (CPU: the plan) and tests/test_gpu_grouped_codebook.py.

- ``CASES``: the smallest shapes at which a workgroup changes tables in every way it can: a direct call over four groups with a
  short last one, splits that start inside a group, a split that runs through three groups and more, a TB_K step of the tiled
  kernel across a boundary, MFMA steps direct and split, kdim < group_rows and group_rows >= kdim (one group).  Every case runs
  with float32, bf16 and fp16 activations; ``regime_of`` / ``required_regimes``: {stream, tiled, MFMA} x dtype x {direct, split}.
- ``exact_data`` / ``float_data``: group g's centres are offset by 64 g, so a row read from another group's table is off by 64 or
  more per unit of x.  Exact data: integer x, quarter-integer centres, integer bias (cbmm_ref.assert_exact holds; for half x the
  centres are rounded to the dtype first, which keeps them on the quarter grid).
- ``weights``: W[i, o] = centers[i // group_rows][labels[i, o]] (an index >= K reads 0), the centres rounded to ``dtype`` as
  ``centers.to(dtype)`` does when one is given; the reference is cbmm_ref.matmul64 on it.
Test infrastructure only."""
from __future__ import annotations

import itertools

import numpy as np

from . import cbmm_ref, h16_ref

DTYPES = ("f32", "bf16", "fp16")
DT_CODE = {"f32": 0, "bf16": 1, "fp16": 2}    # NNC_DT_* (include/nnc.h)
PATH_STREAM, PATH_TILED, PATH_MFMA = 1, 2, 5
CU_COUNTS = (1, 64, 256, 1024)


def torch_dtype(name):
    import torch

    return {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[name]


def _case(m, kdim, ncols, k, group_rows=32, off=0, x_view=False, bias=True, bias_view=False):
    return dict(m=m, kdim=kdim, ncols=ncols, k=k, group_rows=group_rows, off=off, x_view=x_view, bias=bias, bias_view=bias_view)


CASES = [
    _case(16, 112, 70, 16, off=1),                          # direct, 4 groups, a short last group, unaligned rows
    _case(16, 112, 64, 256, x_view=True),                   # the same walk on aligned rows, K = 256
    _case(1, 112, 70, 3, off=3, bias_view=True),            # 3 splits of 38 rows: two of them start inside a group
    _case(2, 112, 48, 16, bias=False),                      # aligned rows, splits inside groups
    _case(16, 600, 50, 16, group_rows=64, x_view=True),     # stream, 2 splits of 300 rows: 5 and 6 groups each
    _case(8, 300, 40, 256, off=5),                          # stream split, a boundary inside a batch of 8 rows
    _case(17, 112, 130, 16, off=1, x_view=True),            # tiled direct / MFMA direct (one k step per group)
    _case(17, 160, 130, 3, bias_view=True),                 # tiled direct / MFMA split (96 + 64 rows)
    _case(17, 300, 50, 256, off=3),                         # tiled: 2 splits of 150 rows, a TB_K step across row 160; MFMA: 4 splits
    _case(130, 300, 129, 16, group_rows=64, bias=False),    # two row tiles, two column tiles
    _case(4, 20, 50, 16, off=2),                            # kdim < group_rows: one short group
    _case(17, 20, 50, 3),                                   # the same through the tiled kernel and the MFMA tile
    _case(16, 112, 70, 16, group_rows=128),                 # group_rows >= kdim: one group
    _case(17, 300, 50, 256, group_rows=320, off=1),         # one group, split
]


def case_id(c):
    return f"m{c['m']}-kd{c['kdim']}-n{c['ncols']}-k{c['k']}-r{c['group_rows']}-o{c['off']}"


def groups_of(c):
    return -(-c["kdim"] // c["group_rows"])


def regime_of(plan, dtype):
    kernel = {PATH_STREAM: "stream", PATH_TILED: "tiled", PATH_MFMA: "mfma"}[plan["path"]]
    return (kernel, dtype, "split" if plan["splits"] > 1 else "direct")


def required_regimes():
    req = set(itertools.product(("stream",), DTYPES, ("direct", "split")))
    req |= set(itertools.product(("tiled",), ("f32",), ("direct", "split")))
    req |= set(itertools.product(("mfma",), ("bf16", "fp16"), ("direct", "split")))
    return req


def split_ranges(plan, kdim):
    return [(s * plan["rps"], min(kdim, (s + 1) * plan["rps"])) for s in range(plan["splits"])]


def round_centres(cen, dtype):
    return np.asarray(cen, dtype=np.float32) if dtype == "f32" else h16_ref.round_to(cen, dtype).reshape(np.shape(cen))


def weights(cen, lab, kdim, ncols, group_rows, dtype="f32"):
    """W (kdim, ncols) float32 from centres (G, K) and indices: an index >= K reads 0."""
    cen = round_centres(cen, dtype)
    k = cen.shape[1]
    table = np.concatenate([cen, np.zeros((cen.shape[0], 1), dtype=np.float32)], axis=1)
    lab = np.minimum(np.asarray(lab).reshape(kdim, ncols), k)
    return table[(np.arange(kdim) // group_rows)[:, None], lab]


def exact_data(c, seed):
    """labels, integer x, quarter-integer centres offset by 64 g, integer bias (or None)."""
    rng = np.random.RandomState(seed)
    g = groups_of(c)
    lab = rng.randint(0, c["k"], size=c["kdim"] * c["ncols"])
    x = rng.randint(-4, 5, size=(c["m"], c["kdim"])).astype(np.float32)
    cen = (rng.randint(-16, 17, size=(g, c["k"])) / 4.0 + 64.0 * np.arange(g)[:, None]).astype(np.float32)
    bias = rng.randint(-50, 51, size=c["ncols"]).astype(np.float32) if c["bias"] else None
    return lab, x, cen, bias


def float_data(c, seed):
    rng = np.random.RandomState(seed + 1)
    g = groups_of(c)
    x = rng.standard_normal((c["m"], c["kdim"])).astype(np.float32)
    cen = (rng.standard_normal((g, c["k"])) + 64.0 * np.arange(g)[:, None]).astype(np.float32)
    bias = rng.standard_normal(c["ncols"]).astype(np.float32) if c["bias"] else None
    return x, cen, bias


def reference(x, w, bias=None):
    return cbmm_ref.matmul64(x, w, bias)
