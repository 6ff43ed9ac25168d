"""The stream instantiations of the backward units of the byte, bitmap-sparse and grouped index forms, and one case list that reaches
every one of them, shared by tests/test_backward_stream_cells_abi.py (CPU: the plans, the tables against the
sources) and tests/test_gpu_training_backward_stream_cells.py.

For m <= 16 every backward call runs a stream kernel picked from a table of template instantiations.  A *cell* is one entry of such
a table, times aligned / unaligned label rows where the kernel is compiled for both:

- byte form (csrc/nnc_cbgrad.hip float32, csrc/nnc_cbgrad_h16.hip bf16 / fp16): (label bytes, vb, mt, aligned), 20 cells;
- bitmap-sparse form (csrc/nnc_cbspgrad.hip, csrc/nnc_cbspgrad_h16.hip): (label bytes, mt), 10 cells;
- grouped form (csrc/nnc_cbgrad_grouped.hip, csrc/nnc_cbgrad_grouped_h16.hip; uint8 only): (vb, mt, aligned), 10 cells.

``BYTE_TABLE`` / ``SPARSE_TABLE`` / ``GROUPED_TABLE`` are the tables, hard-coded; ``UNITS`` names the six units and the element types
each runs with.  ``CASES[form]`` holds one case per cell x m x width:

- m: the smallest and the largest m that select the cell's mt (``MS_OF_MT``); with m < mt the rows r >= m add nothing and are not stored.
- byte and grouped: E = vb / label bytes labels a lane, kdim = 93 (three row groups of 31: waves 0-2 take one unrolled batch of 8
  rows, wave 3 the tail loop of 7, at any CU count); ncols = 3 E (one column block: the direct store) or 67 E (two blocks, the last
  one ragged: the partials and k_cbgrad_reduce), + 1 for unaligned rows, or the aligned width one element into its buffer.  K = 200
  (uint8) / 300 (uint16); grouped: K = 16, group_rows = 32 (three groups, the last of 29 rows, a workgroup in two of them).  The
  unaligned cases hold indices >= K.
- sparse: kdim = 300, ncols = 64 segs - 3 (one block) or 64 segs + 3 (two), segs = ``SEGS_OF_MT``; density 0.3; the skipped symbol
  is given and its centre is 0.75, so the rank-1 term runs.

Every case states what its plans must report (``expect``); the ABI test asserts it at 80, 256 and 304 CUs.

``data(case, dtype)``: the exact data of the existing references (``cbgrad_ref.case_data``, ``sparse_grad_ref.case_data``,
``grouped_grad_ref.exact_data`` / ``labels_of``: integer x and g in [-3, 3], quarter-integer centres, grouped centres offset by
64 q) and their float64 formulas, computed once per (case, dtype) and shared; the arrays are read-only.  With a half dtype the
centres are rounded to it first (``h16_ref.round_to``), as the kernels do: a no-op but for the grouped offsets.  The precondition of
"bit for bit" is asserted there: four times the largest sum of magnitudes (the sums counted in quarters) is below 2^24, so every
partial sum in any order is an exact float32.
Test infrastructure only."""
from __future__ import annotations

import functools

import numpy as np

from . import cbgrad_ref, grouped_grad_ref, sparse_grad_ref
from .h16_ref import round_to, torch_dtype

PATH_STREAM = cbgrad_ref.PATH_STREAM
CU_COUNTS = (80, 256, 304)
DTYPES = ("f32", "bf16", "fp16")

# ------------------------------------------------------------------ the tables of instantiations
# byte form: (label bytes, vb, mt), each compiled aligned and unaligned (CBG_U8_STREAM_CASES / CBG_U16_STREAM_CASES of nnc_cbgrad.hpp)
BYTE_TABLE = ((1, 16, 1), (1, 16, 2), (1, 16, 4), (1, 8, 8), (1, 4, 16), (2, 16, 1), (2, 16, 2), (2, 16, 4), (2, 16, 8), (2, 8, 16))
# sparse form: (label bytes, mt) (SG_CASE of nnc_cbspgrad.hip, SGH_CASE of nnc_cbspgrad_h16.hip)
SPARSE_TABLE = ((1, 1), (1, 2), (1, 4), (1, 8), (1, 16), (2, 1), (2, 2), (2, 4), (2, 8), (2, 16))
# grouped form: (vb, mt), each compiled aligned and unaligned (CBG_U8_STREAM_CASES)
GROUPED_TABLE = ((16, 1), (16, 2), (16, 4), (8, 8), (4, 16))

BYTE_CELLS = frozenset((lb, vb, mt, a) for lb, vb, mt in BYTE_TABLE for a in (1, 0))
SPARSE_CELLS = frozenset(SPARSE_TABLE)
GROUPED_CELLS = frozenset((vb, mt, a) for vb, mt in GROUPED_TABLE for a in (1, 0))
CELLS = {"byte": BYTE_CELLS, "sparse": SPARSE_CELLS, "grouped": GROUPED_CELLS}

# the six units: form, the element types it runs with, its source
UNITS = {
    "byte_f32": ("byte", ("f32",), "nnc_cbgrad.hip"),
    "byte_h16": ("byte", ("bf16", "fp16"), "nnc_cbgrad_h16.hip"),
    "sparse_f32": ("sparse", ("f32",), "nnc_cbspgrad.hip"),
    "sparse_h16": ("sparse", ("bf16", "fp16"), "nnc_cbspgrad_h16.hip"),
    "grouped_f32": ("grouped", ("f32",), "nnc_cbgrad_grouped.hip"),
    "grouped_h16": ("grouped", ("bf16", "fp16"), "nnc_cbgrad_grouped_h16.hip"),
}

MS_OF_MT = {1: (1,), 2: (2,), 4: (3, 4), 8: (5, 8), 16: (9, 16)}
SEGS_OF_MT = {1: 8, 2: 8, 4: 8, 8: 4, 16: 2}
SPARSE_ROW_TILES = {8: 10, 4: 5, 2: 3}     # kdim 300 over batches of 4 waves x 64 / segs rows
KDIM, SPARSE_KDIM = 93, 300
K_OF_LB = {1: 200, 2: 300}
GROUPED_K, GROUP_ROWS = 16, 32
SPARSE_Z, SPARSE_DENSITY = 5, 0.3
# (variant, columns past a multiple of E, label offset in elements): aligned; a width that leaves rows unaligned; an unaligned address
VARIANTS = (("aligned", 0, 0), ("width", 1, 0), ("address", 0, 1))
WIDTHS = (("one", 3), ("two", 67))          # column blocks, multiples of E


def _dense_cases(form):
    cases = []
    table = BYTE_TABLE if form == "byte" else tuple((1, vb, mt) for vb, mt in GROUPED_TABLE)
    for lb, vb, mt in table:
        e = vb // lb
        for m in MS_OF_MT[mt]:
            for wname, mult in WIDTHS:
                for variant, extra, off in VARIANTS:
                    ncols = mult * e + extra
                    blocks = -(-ncols // (64 * e))
                    c = dict(form=form, lb=lb, vb=vb, mt=mt, m=m, kdim=KDIM, ncols=ncols, off=off, aligned=int(variant == "aligned"),
                             oob=variant != "aligned", k=K_OF_LB[lb] if form == "byte" else GROUPED_K,
                             id=f"u{8 * lb}-vb{vb}-mt{mt}-m{m}-{wname}-{variant}",
                             expect={"dx": dict(col_tiles=blocks, splits=blocks, row_tiles=3), "dc": dict(col_tiles=blocks, splits=1, row_tiles=3)})
                    if form == "grouped":
                        c["group_rows"] = GROUP_ROWS
                        for p in c["expect"].values():
                            p.update(groups=3, rows_per_group=31, max_groups_per_workgroup=2)
                    assert blocks == (1 if wname == "one" else 2)
                    cases.append(c)
    return cases


def _sparse_cases():
    cases = []
    for lb, mt in SPARSE_TABLE:
        segs = SEGS_OF_MT[mt]
        for m in MS_OF_MT[mt]:
            for wname, extra in (("one", -3), ("two", 3)):
                blocks = 1 if wname == "one" else 2
                rt = SPARSE_ROW_TILES[segs]
                cases.append(dict(form="sparse", lb=lb, mt=mt, segs=segs, m=m, kdim=SPARSE_KDIM, ncols=64 * segs + extra, k=K_OF_LB[lb],
                                  z=SPARSE_Z, oob=wname == "two", id=f"u{8 * lb}-mt{mt}-m{m}-{wname}",
                                  expect={"dx": dict(col_tiles=blocks, splits=blocks, row_tiles=rt), "dc": dict(col_tiles=blocks, splits=1, row_tiles=rt)}))
    return cases


CASES = {"byte": _dense_cases("byte"), "sparse": _sparse_cases(), "grouped": _dense_cases("grouped")}
BY_ID = {form: {c["id"]: c for c in cases} for form, cases in CASES.items()}


def cell_of(case):
    """The table cell the case is built for."""
    if case["form"] == "byte":
        return (case["lb"], case["vb"], case["mt"], case["aligned"])
    if case["form"] == "sparse":
        return (case["lb"], case["mt"])
    return (case["vb"], case["mt"], case["aligned"])


def cell_of_plan(case, plan):
    """The cell a dx or dc plan of the case's unit reports (the label width is the call's own argument)."""
    if case["form"] == "byte":
        return (case["lb"], plan["vb"], plan["mt"], plan["aligned"])
    if case["form"] == "sparse":
        return (case["lb"], plan["mt"])
    return (plan["vb"], plan["mt"], plan["aligned"])


def labels_addr(case, base=256):
    """The address of the labels in a buffer at ``base``: ``off`` elements in."""
    return base + case.get("off", 0) * case["lb"]


def plans(case, dtype, cus, addr=None):
    """(dx plan, dc plan, dx workspace bytes, dc workspace bytes) of the case's unit for ``dtype`` on ``cus`` compute units, the labels at
    ``addr`` (default: ``labels_addr(case)``).  Host only."""
    from neural_network_compression_amd import _native as nat
    from neural_network_compression_amd import ops

    lib = nat.load()
    m, kdim, ncols, k, form = case["m"], case["kdim"], case["ncols"], case["k"], case["form"]
    h = dtype != "f32"
    sfx = "_h16" if h else ""
    pre = (torch_dtype(dtype),) if h else ()
    addr = labels_addr(case) if addr is None else addr
    if form == "byte":
        args = (m, kdim, ncols, case["lb"], k, cus, addr)
        names, ws_args = "cbmm", ((m, kdim, ncols, case["lb"]), (m, kdim, ncols, case["lb"], k))
    elif form == "sparse":
        args = (m, kdim, ncols, case["lb"], k, cus)
        names, ws_args = "cbsp", ((m, kdim, ncols, case["lb"]), (m, kdim, ncols, case["lb"], k))
    else:
        args = (m, kdim, ncols, k, case["group_rows"], cus, addr)
        names, ws_args = "cbmm_grouped", ((m, kdim, ncols), (m, kdim, ncols, k, case["group_rows"]))
    dx = getattr(ops, f"{names}_dx{sfx}_plan")(*pre, *args)
    dc = getattr(ops, f"{names}_dc{sfx}_plan")(*pre, *args)
    return (dx, dc, int(getattr(lib, f"nnc_{names}_dx{sfx}_workspace_bytes")(*ws_args[0])),
            int(getattr(lib, f"nnc_{names}_dc{sfx}_workspace_bytes")(*ws_args[1])))


# ------------------------------------------------------------------ data and references
def _seed(case):
    return 1 + CASES[case["form"]].index(BY_ID[case["form"]][case["id"]])


def assert_exact(*magnitudes):
    """The precondition of the bit-for-bit comparisons: four times every sum of magnitudes (so the sum counted in quarters, the unit
    of the centres) stays below 2^24, and with it every partial sum of the same terms in any order is an exact float32."""
    top = max(float(np.max(m, initial=0.0)) for m in magnitudes)
    assert 4.0 * top < 2.0 ** 24, top
    return top


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _data(form, case_id, dtype):
    case = BY_ID[form][case_id]
    m, kdim, ncols, k = case["m"], case["kdim"], case["ncols"], case["k"]
    rnd = (lambda c: c) if dtype == "f32" else (lambda c: round_to(c, dtype))
    if form == "byte":
        x, g, c, lab = cbgrad_ref.case_data((case_id, m, kdim, ncols, case["lb"], k, case["off"], case["oob"]), _seed(case))
        ch = rnd(c)
        out = dict(x=x, g=g, centers=c, labels=lab, dx=cbgrad_ref.dx64(g, lab, ch), dc=cbgrad_ref.dc64(x, g, lab, k))
        mag = np.abs(g).astype(np.float64) @ np.abs(cbgrad_ref.decoded(lab, ch)).T
    elif form == "sparse":
        tup = (case_id, m, kdim, ncols, case["lb"], k, SPARSE_DENSITY, case["z"], case["oob"], False)
        x, g, c, lab, z = sparse_grad_ref.case_data(tup, _seed(case))
        assert z == case["z"] and c[z] == 0.75
        ch = rnd(c)
        out = dict(x=x, g=g, centers=c, labels=lab, dx=sparse_grad_ref.dx64(g, lab, ch, z), dc=cbgrad_ref.dc64(x, g, lab, k))
        D, cz = sparse_grad_ref.stored_d(lab, ch, z)
        ga = np.abs(g).astype(np.float64)
        mag = ga @ np.abs(D).T + abs(cz) * ga.sum(axis=1, keepdims=True)
    else:
        x, g, c = grouped_grad_ref.exact_data(case, _seed(case))
        lab = grouped_grad_ref.labels_of(case, _seed(case), oob=case["oob"])
        ch = rnd(c)
        out = dict(x=x, g=g, centers=c, labels=lab, dx=grouped_grad_ref.dx64(case, g, lab, ch), dc=grouped_grad_ref.dc64(case, x, g, lab))
        mag = np.abs(g).astype(np.float64) @ np.abs(grouped_grad_ref.decoded(case, lab, ch)).T
    if case["oob"]:
        assert (lab >= k).any()
    # dx: sum_o |g| |W| per element; dc: sum_r |x| |g| per dW (the bins are integer sums of the exact dW, whatever their size)
    out["top"] = assert_exact(mag, np.abs(x).astype(np.float64).T @ np.abs(g).astype(np.float64))
    return _frozen(out)


def data(case, dtype):
    """dict(x, g, centers, labels, dx, dc[, top]): the inputs (float32 / int64, read-only, shared) and the float64 results of the unit run with
    ``dtype`` ("f32", "bf16", "fp16").  dc has the unit's shape: [K], or [G, K] for the grouped form."""
    return _data(case["form"], case["id"], dtype)
