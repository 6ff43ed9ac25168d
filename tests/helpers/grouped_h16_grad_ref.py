"""The case list and the data of the group-wise codebook backward tests on bf16 / fp16 activations (nnc_cbmm_grouped_dx_h16 /
nnc_cbmm_grouped_dc_h16, csrc/nnc_cbgrad_grouped_h16.hip), shared by tests/test_grouped_codebook_grad_h16_abi.py
(CPU: the plans) and tests/test_gpu_grouped_codebook_backward_h16.py.

- ``CASES``: (m, kdim, ncols, K, group_rows, label offset, x and g as buf[1:] views): the smallest shapes at which the walk through
  the groups can go wrong.  kdim 300 at group_rows 32 gives 128-row tiles with 4, 4 and 2 groups and a last group of 12 rows; kdim
  200 at group_rows 96 a boundary off every multiple of 128; kdim 256 at group_rows 128 one group per tile; group_rows >= kdim one
  group.  ncols 50 is one split of dx, 130 two (element arm), 128 two with g 16-byte aligned (XVEC); m 1, 5, 16 run the stream
  kernels, 17, 64, 130 the MFMA ones (130 splits m in dc).  Every case runs with both dtypes.  G * K stays <= 1040, so the dc
  identity with codebook_centroid_grad applies to every case.
- ``regime_of`` / ``REQUIRED``: the cell {stream, mfma} x {direct, split} a plan lies in, and the cells the list has to hit.
- ``exact_data``: integer x and g in [-3, 3] and centres n / 4 + 4 q, all exact in bf16 and fp16, every sum an exact float32.
- ``float_data``: randn x, 0.01 randn g, centres 0.08 * sorted randn scaled by 1 + q per group.
Test infrastructure only."""
from __future__ import annotations

import numpy as np

from . import cbgrad_ref, grouped_grad_ref
from .h16_ref import DTYPES, PATH_MFMA, PATH_STREAM

CU_COUNTS = (1, 80, 256, 1024)


def _case(m, kdim, ncols, k, group_rows, off=0, view=False):
    return dict(m=m, kdim=kdim, ncols=ncols, k=k, group_rows=group_rows, off=off, view=view)


STREAM_CASES = [
    _case(1, 300, 50, 16, 32),
    _case(5, 200, 130, 3, 96, 1, True),
    _case(16, 300, 130, 16, 32, 3, True),
    _case(16, 200, 300, 16, 96),              # two column blocks at mt 16: the dx partials go through the reduce
    _case(16, 256, 128, 256, 128),
]
MFMA_CASES = [
    _case(17, 300, 130, 16, 32, 1),           # tiles over 4, 4 and 2 groups; ncols split in two, element arm
    _case(64, 300, 128, 3, 32),               # XVEC: g 16-byte aligned, ncols a multiple of 8; x and g 4-byte aligned
    _case(130, 200, 50, 256, 96, 0, True),    # m split in two in dc, dx direct; tiles over groups {0, 1}, {1, 2}; K = 256
    _case(17, 256, 50, 1, 128),               # one group per tile, K = 1
    _case(64, 200, 130, 16, 96, 1),
    _case(17, 256, 128, 256, 128),            # the m = 17 twin of the last stream case
]
ONE_GROUP_CASES = [_case(5, 200, 50, 16, 224, 1), _case(17, 200, 130, 256, 512, 0, True), _case(130, 300, 128, 3, 320)]
CASES = STREAM_CASES + MFMA_CASES + ONE_GROUP_CASES
EMPTY_CASES = [_case(0, 50, 60, 8, 32), _case(4, 0, 60, 8, 32), _case(20, 0, 60, 8, 32), _case(4, 50, 0, 8, 32), _case(20, 50, 0, 8, 32)]


# the packed form: the same shapes with K <= 2^bits; K in {1, 3, 4} at 2 bits, {5, 16} at 4 bits; labels >= K wherever K < 2^bits
PACKED_CASES = [
    dict(_case(1, 300, 50, 3, 32), bits=2),
    dict(_case(5, 200, 130, 5, 96, 0, True), bits=4),
    dict(_case(16, 300, 300, 16, 32, 0, True), bits=4),   # two column blocks: the dx partials go through the reduce
    dict(_case(16, 200, 300, 4, 96), bits=2),
    dict(_case(17, 300, 130, 16, 32), bits=4),
    dict(_case(64, 300, 128, 3, 32), bits=2),
    dict(_case(130, 200, 50, 5, 96, 0, True), bits=4),
    dict(_case(17, 256, 50, 1, 128), bits=2),
    dict(_case(130, 200, 130, 4, 96), bits=2),
    dict(_case(5, 200, 50, 16, 224), bits=4),            # one group
    dict(_case(17, 200, 130, 3, 512, 0, True), bits=2),  # one group
    dict(_case(130, 300, 128, 5, 320), bits=4),          # one group
]


def packed_labels_of(c, seed):
    """(kdim, ncols) indices in [0, 2^bits): beyond K wherever the field has room."""
    return np.random.RandomState(seed).randint(0, 1 << c["bits"], size=(c["kdim"], c["ncols"]))


def packed_case_id(c):
    return f"b{c['bits']}-" + case_id(c)


def case_id(c):
    return f"m{c['m']}-kd{c['kdim']}-n{c['ncols']}-k{c['k']}-r{c['group_rows']}-o{c['off']}" + ("-view" if c["view"] else "")


groups_of = grouped_grad_ref.groups_of
group_rows_of = grouped_grad_ref.group_rows_of
labels_of = grouped_grad_ref.labels_of
labels16 = grouped_grad_ref.labels16


def regime_of(plan):
    assert plan["path"] in (PATH_STREAM, PATH_MFMA), plan
    return ("stream" if plan["path"] == PATH_STREAM else "mfma", "split" if plan["splits"] > 1 else "direct")


REQUIRED = {"dx": {("stream", "direct"), ("stream", "split"), ("mfma", "direct"), ("mfma", "split")},
            "dc": {("stream", "direct"), ("mfma", "direct"), ("mfma", "split")}}   # (section 12's stream dc plan never splits m)


def tile_tables(group_rows):
    """The tables / sets of bins a 128-row tile holds: tiles start on multiples of 128, group_rows is a multiple of 32."""
    return 1 if group_rows % 128 == 0 else (4 if group_rows == 32 else 2)


def exact_data(c, seed):
    rng = np.random.RandomState(seed + 17)
    x = rng.randint(-3, 4, size=(c["m"], c["kdim"])).astype(np.float32)
    g = rng.randint(-3, 4, size=(c["m"], c["ncols"])).astype(np.float32)
    G = groups_of(c)
    cen = (rng.randint(-8, 9, size=(G, c["k"])) / 4.0 + 4.0 * np.arange(G)[:, None]).astype(np.float32)
    return x, g, cen


def float_data(c, seed):
    rng = np.random.RandomState(seed + 29)
    x = rng.standard_normal((c["m"], c["kdim"])).astype(np.float32)
    g = (rng.standard_normal((c["m"], c["ncols"])) * 1e-2).astype(np.float32)
    G = groups_of(c)
    cen = (0.08 * np.sort(rng.standard_normal((G, c["k"])), axis=1) * (1.0 + np.arange(G))[:, None]).astype(np.float32)
    return x, g, cen


def dx64(c, g, lab, cen):
    return grouped_grad_ref.dx64(c, g, lab, cen)


def dc64(c, x, g, lab):
    return grouped_grad_ref.dc64(c, x, g, lab)


__all__ = ["CASES", "DTYPES", "cbgrad_ref"]
