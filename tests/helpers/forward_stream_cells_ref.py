"""The stream instantiations of the forward codebook units, and one case list per unit that reaches every one of them in both modes
(DESIGN.md section 33), shared by tests/test_forward_stream_cells_abi.py (CPU: the plans, the tables against the sources) and
tests/test_gpu_zz_forward_stream_cells.py.  The half-precision backward units of the 2- and 4-bit packed form, grouped and not, which section 29 left out, are here too.

For m <= 16 every codebook product runs a stream kernel picked from a table of template instantiations.  A *cell* is one entry of
such a table, times aligned / unaligned label rows where the kernel is compiled for both:

- byte form, bf16 / fp16 (csrc/nnc_cbmm_h16.hip, H16_STREAM_CASES): (label bytes, vb, mt, aligned), 20 cells;
- bitmap-sparse form, bf16 / fp16 (csrc/nnc_cbsp_h16.hip, SP_H16_STREAM_CASES): (label bytes, mt), 10 cells;
- grouped byte form, float32 / bf16 / fp16 (csrc/nnc_cbmm_grouped.hip, GROUPED_STREAM_CASES): (vb, mt, aligned), 10 cells;
- packed form, float32 (csrc/nnc_cbpk.hip, PK_CASE) and grouped packed form, float32 / bf16 / fp16 (csrc/nnc_cbpk_grouped.hip,
  PKG_STREAM_CASES; nnc_cbpk_h16 is that unit with one group): (bits, vb, mt), 18 cells;
- packed backward, bf16 / fp16 (csrc/nnc_cbpk_h16.hip over PKG_STREAM_CASES of nnc_cbpkgrad.hpp) and grouped packed backward, bf16 / fp16
  (csrc/nnc_cbpkgrad_grouped_h16.hip over the same list): (bits, vb, mt), 18 cells.

``TABLES`` holds them hard-coded (and those of the three forward units whose older case lists are already complete, so that the ABI
test compares every source list with a table).  ``CASES[form]`` holds the cases; each states the cell it is built for, its mode
("direct": one split, the kernel stores y itself; "split": the float32 partials and k_cbmm_reduce) and what the plan must report
(``expect``: col_tiles and, for the grouped forms, groups; ``split_of`` / ``groups_in_a_split``: splits, rows per split and
max_groups_per_split, from the rules the sources state; ``check_plan`` asserts all of it).  The forward splits along kdim, so every
cell has cases of both modes:

- m: the smallest and the largest m that select the cell's mt (``stream_cells_ref.MS_OF_MT``).
- kdim: 31 and 61 are direct at every m (kdim / 32 < 2); 31 gives waves 0-2 one unrolled batch of 8 rows and wave 3 the tail loop of
  7, 61 gives two batches, and one batch plus a tail of 5.  The split kdim is the first odd one from max(64, 32 mt / label bytes) + 29 on (packed:
  max(64, 64 mt / bits) + 29; sparse: 541) with two splits or more and a ragged last one at every m of the mt (``ragged_kdim``).  A group-wise layer with three groups cannot be
  direct at m <= 2 (group_rows >= 32, and kdim >= 64 splits there), so the direct grouped cases have one group (kdim 31) and two
  with a short last one (61: the boundary inside the workgroup); the split ones have three groups or more, a short last one, and a
  boundary inside a split.
- widths and alignment, byte and grouped: those of section 29 (3 E and 67 E columns, + 1 column, or one element into the buffer);
  the unaligned cases hold indices >= K.  K = 200 (uint8), 300 (uint16); grouped: K = 16, group_rows = 32.
- sparse: 61 and 67 columns (one block and two), density 0.3, the skipped symbol's centre is 0.75; the two-block cases hold stored
  symbols >= K.
- packed: vb <= 4 comes from narrow shapes (64 cols - 5 and 64 cols + 37 columns: both leave padding fields in the last 16-byte
  group).  vb 8 and 16 are planned only where column tiles x s_max >= 256 (pk_plan), so a direct case of such a cell needs 256
  column tiles and a split case kdim >= 32 * 256 / tiles: ``WIDE`` holds, per cell, the smallest kdim x ncols a search of the plan
  found (6.7 to 32 million indices, 3.4 to 8.1 MB of packed bytes; the second direct kdim would double them and is left out there).
  K alternates between 2^bits and a smaller K with labels >= K.  The grouped packed cases have three groups with a short last one
  where kdim allows it (as above).
- the epilogue rotates over the cases of each (cell, mode): bias present / absent, ReLU on (the pre-activations have both signs:
  asserted) / off.  A half unit runs every case with y as float32 and as the half type, so every cell sees ``direct`` 1 and 2 and
  both output types of the reduce.

``data(case, dtype)``: integer x in [-3, 3], quarter-integer centres in [-2, 2] (grouped byte: +- 64 per group, rounded to the half
type first as the kernels do; grouped packed: +- 16 per group, exact in bf16, so one float64 product serves the three element
types), integer bias in [-50, 50]; the float64 product, computed once and shared, read-only.  The precondition of "bit for bit" is
asserted there (``stream_cells_ref.assert_exact``): four times the largest sum of magnitudes, bias included, is below 2^24.
Test infrastructure only."""
from __future__ import annotations

import functools

import numpy as np

from . import packed_ref, stream_cells_ref
from .h16_ref import round_to
from .sparse_ref import labels_at_density
from .stream_cells_ref import MS_OF_MT, assert_exact

PATH_STREAM = 1
CU_COUNTS = (80, 256, 304)
PLAN_CUS = 256                                  # CB_PLAN_CUS: no plan splits for more CUs than this

# ------------------------------------------------------------------ the tables of instantiations
PACKED_TABLE = ((4, 16, 1), (4, 16, 2), (4, 8, 1), (4, 8, 2), (4, 8, 4), (4, 4, 1), (4, 4, 2), (4, 4, 4), (4, 4, 8), (4, 2, 16),
                (2, 16, 1), (2, 8, 1), (2, 8, 2), (2, 4, 1), (2, 4, 2), (2, 4, 4), (2, 2, 8), (2, 1, 16))
TABLES = {
    "byte": stream_cells_ref.BYTE_TABLE,        # (label bytes, vb, mt): kStreamCases of nnc_cbmm.hip, H16_STREAM_CASES
    "sparse": stream_cells_ref.SPARSE_TABLE,    # (label bytes, mt): kSpStreamCases of nnc_cbsp.hip, SP_H16_STREAM_CASES
    "grouped": stream_cells_ref.GROUPED_TABLE,  # (vb, mt): GROUPED_STREAM_CASES
    "packed": PACKED_TABLE,                     # (bits, vb, mt): the PK_CASE list, PKG_STREAM_CASES (forward and backward)
    "gsparse": (1, 2, 4, 8, 16),                # mt: SPG_STREAM_CASES, kSggCases
}
CELLS = {
    "byte": frozenset((lb, vb, mt, a) for lb, vb, mt in TABLES["byte"] for a in (1, 0)),
    "sparse": frozenset(TABLES["sparse"]),
    "grouped": frozenset((vb, mt, a) for vb, mt in TABLES["grouped"] for a in (1, 0)),
    "packed": frozenset(PACKED_TABLE),
    "gpacked": frozenset(PACKED_TABLE),
    "packed_bwd": frozenset(PACKED_TABLE),
    "gpacked_bwd": frozenset(PACKED_TABLE),
}
# unit -> (form, element types, source)
UNITS = {
    "byte_h16": ("byte", ("bf16", "fp16"), "nnc_cbmm_h16.hip"),
    "sparse_h16": ("sparse", ("bf16", "fp16"), "nnc_cbsp_h16.hip"),
    "grouped": ("grouped", ("f32", "bf16", "fp16"), "nnc_cbmm_grouped.hip"),
    "packed_f32": ("packed", ("f32",), "nnc_cbpk.hip"),
    "gpacked": ("gpacked", ("f32", "bf16", "fp16"), "nnc_cbpk_grouped.hip"),
    "packed_bwd_h16": ("packed_bwd", ("bf16", "fp16"), "nnc_cbpk_h16.hip"),
    "gpacked_bwd_h16": ("gpacked_bwd", ("bf16", "fp16"), "nnc_cbpkgrad_grouped_h16.hip"),
}

K_OF_LB = {1: 200, 2: 300}
GROUPED_K, GROUP_ROWS = 16, 32
SPARSE_Z, SPARSE_DENSITY, SPARSE_SPLIT_KDIM = 5, 0.3, 541
SMALL_K = {4: 5, 2: 3}
VARIANTS = stream_cells_ref.VARIANTS
WIDTHS = stream_cells_ref.WIDTHS
DIRECT_KDIMS = (31, 61)
# (bits, vb, mt) -> ((kdim, ncols) direct, (least kdim, ncols) split): the smallest kdim x ncols of each mode at which pk_plan picks the cell;
# the split kdim is the first odd one from there on with a ragged last split (ragged_kdim)
WIDE = {
    (4, 16, 1): ((31, 522241), (4097, 3277)), (4, 16, 2): ((31, 522241), (4097, 3277)),
    (4, 8, 1): ((31, 261121), (2049, 3277)), (4, 8, 2): ((31, 261121), (2049, 3277)), (4, 8, 4): ((31, 261121), (2049, 3277)),
    (2, 16, 1): ((31, 1044481), (8193, 3277)), (2, 8, 1): ((31, 522241), (4097, 3277)), (2, 8, 2): ((31, 522241), (4097, 3277)),
}
# the packed backward plans (pg_stream_grid) ask for column blocks x row groups >= 512: the shapes of grouped_packed_grad_ref.WIDE_CASES
WIDE_BWD = {(4, 8, 1): (16400, 1024), (4, 8, 2): (16400, 1024), (4, 8, 4): (16400, 1024), (4, 16, 1): (16400, 2048),
            (4, 16, 2): (16400, 2048), (2, 8, 1): (16400, 2048), (2, 8, 2): (16400, 2048), (2, 16, 1): (16400, 4096)}


def cdiv(a, b):
    return -(-a // b)


def _split(kdim, s):
    """(splits, rows per split) of a kernel that was offered ``s`` splits"""
    rps = cdiv(kdim, max(1, s))
    return cdiv(kdim, rps), rps


def _split_for(form, m, kdim, width, ct, cus):
    """(splits, rows per split) by the rules the sources state (two workgroups per CU, four for the sparse form; a batch of rows per
    wave; the partials within a share of the index stream); ``width``: the label bytes, or the bits of a packed index"""
    cus = min(cus, PLAN_CUS)
    if form in ("byte", "grouped"):
        return _split(kdim, min(cdiv(2 * cus, ct), kdim // 32, kdim * width // (16 * m)))
    if form == "sparse":
        return _split(kdim, min(cdiv(4 * cus, ct), kdim // 256, kdim // (16 * m)))
    return _split(kdim, min(cdiv(2 * cus, ct), max(1, min(kdim // 32, kdim * width // (32 * m)))))


def split_of(case, cus):
    """What the case claims of the plan at ``cus`` compute units: (splits, rows per split)"""
    return _split_for(case["form"], case["m"], case["kdim"], case.get("lb", case.get("bits")), case["expect"]["col_tiles"], cus)


def ragged_kdim(form, mt, width, ct, start):
    """The first odd kdim >= ``start`` that every m of ``mt`` splits, at each of CU_COUNTS, with a ragged last split"""
    for kdim in range(start | 1, start + 400, 2):
        got = [_split_for(form, m, kdim, width, ct, cus) for m in MS_OF_MT[mt] for cus in CU_COUNTS]
        if all(s >= 2 and kdim % rps for s, rps in got):
            return kdim
    raise AssertionError((form, mt, width, ct, start))


def groups_in_a_split(case, cus):
    splits, rps = split_of(case, cus)
    gr, kdim = case["group_rows"], case["kdim"]
    return max((min(kdim, lo + rps) - 1) // gr - lo // gr + 1 for lo in range(0, splits * rps, rps))


class _Rotation:
    """bias / ReLU of the j-th case of a (cell, mode): the split cases start three steps in, so a cell with one case a mode sees both of each"""

    def __init__(self):
        self.seen = {}

    def next(self, cell, mode):
        j = self.seen.get((cell, mode), 3 if mode == "split" else 0)
        self.seen[(cell, mode)] = j + 1
        return dict(bias=j % 2 == 0, relu=j % 4 < 2, j=j)


def _modes(split_kdim):
    return (("direct", DIRECT_KDIMS[0]), ("direct", DIRECT_KDIMS[1]), ("split", split_kdim))


def _dense_cases(form):
    cases, rot = [], _Rotation()
    table = TABLES["byte"] if form == "byte" else tuple((1, vb, mt) for vb, mt in TABLES["grouped"])
    for lb, vb, mt in table:
        e = vb // lb
        for m in MS_OF_MT[mt]:
            for mode, kdim in _modes(max(ragged_kdim(form, mt, lb, ct, max(64, 32 * mt // lb) + 29) for ct in (1, 2))):
                for wname, mult in WIDTHS:
                    for variant, extra, off in VARIANTS:
                        ncols = mult * e + extra
                        aligned = int(variant == "aligned")
                        cell = (lb, vb, mt, aligned) if form == "byte" else (vb, mt, aligned)
                        c = dict(form=form, cell=cell, lb=lb, vb=vb, mt=mt, m=m, kdim=kdim, ncols=ncols, off=off, aligned=aligned, mode=mode,
                                 oob=not aligned, k=K_OF_LB[lb] if form == "byte" else GROUPED_K,
                                 id=f"u{8 * lb}-vb{vb}-mt{mt}-m{m}-kd{kdim}-{wname}-{variant}", expect=dict(col_tiles=cdiv(ncols, 64 * e)),
                                 **rot.next(cell, mode))
                        assert c["expect"]["col_tiles"] == (1 if wname == "one" else 2)
                        if form == "grouped":
                            c["group_rows"] = GROUP_ROWS
                            c["expect"]["groups"] = cdiv(kdim, GROUP_ROWS)
                        cases.append(c)
    return cases


def _sparse_cases():
    cases, rot = [], _Rotation()
    for lb, mt in TABLES["sparse"]:
        for m in MS_OF_MT[mt]:
            for mode, kdim in (("direct", 31), ("direct", 300), ("split", SPARSE_SPLIT_KDIM)):
                for wname, ncols in (("one", 61), ("two", 67)):
                    cases.append(dict(form="sparse", cell=(lb, mt), lb=lb, mt=mt, m=m, kdim=kdim, ncols=ncols, k=K_OF_LB[lb], z=SPARSE_Z, mode=mode,
                                      oob=wname == "two", id=f"u{8 * lb}-mt{mt}-m{m}-kd{kdim}-{wname}", expect=dict(col_tiles=cdiv(ncols, 64)),
                                      **rot.next((lb, mt), mode)))
    return cases


def group_rows_for(kdim):
    """three groups with a short last one where kdim allows it (a multiple of 32 rows a group)"""
    return max(32, 32 * cdiv(cdiv(kdim, 3), 32))


def _packed_cases(form):
    cases, rot = [], _Rotation()
    for bits, vb, mt in PACKED_TABLE:
        cell, cols = (bits, vb, mt), 8 * vb // bits
        for m in MS_OF_MT[mt]:
            if cell in WIDE:
                (dk, dn), (sk, sn) = WIDE[cell]
                shapes = [("direct", (dk, dn), "wide"), ("split", (ragged_kdim(form, mt, bits, cdiv(sn, 64 * cols), sk), sn), "wide")]
            else:
                shapes = [(mode, (kdim, ncols), wname) for mode, kdim in _modes(max(ragged_kdim(form, mt, bits, ct, max(64, 64 * mt // bits) + 29) for ct in (1, 2)))
                          for wname, ncols in (("one", 64 * cols - 5), ("two", 64 * cols + 37))]
            for mode, (kdim, ncols), wname in shapes:
                r = rot.next(cell, mode)
                k = (1 << bits) if r["j"] % 2 == 0 else SMALL_K[bits]
                c = dict(form=form, cell=cell, bits=bits, vb=vb, mt=mt, m=m, kdim=kdim, ncols=ncols, k=k, oob=k < (1 << bits), mode=mode,
                         wide=wname == "wide", id=f"b{bits}-vb{vb}-mt{mt}-m{m}-kd{kdim}-{wname}", expect=dict(col_tiles=cdiv(ncols, 64 * cols)), **r)
                assert ncols * bits % 128 != 0 or c["wide"]                 # padding fields in the last 16-byte group
                if form == "gpacked":
                    c["group_rows"] = group_rows_for(kdim)
                    c["expect"]["groups"] = cdiv(kdim, c["group_rows"])
                cases.append(c)
    return cases


def _packed_bwd_cases(form):
    """dx splits along ncols (one split a column block), dc never: one block and two for the narrow cells, as section 29; the wide
    cells at the shapes of grouped_packed_grad_ref.WIDE_CASES.  The grouped form: three groups, the last one short."""
    cases = []
    for bits, vb, mt in PACKED_TABLE:
        cell, cols = (bits, vb, mt), 8 * vb // bits
        for m in MS_OF_MT[mt]:
            if cell in WIDE_BWD:
                shapes = [(WIDE_BWD[cell], "wide")]
            else:
                shapes = [((93, 64 * cols - 5), "one"), ((93, 64 * cols + 37), "two")]
            for (kdim, ncols), wname in shapes:
                j = len(cases)
                k = (1 << bits) if j % 2 == 0 else SMALL_K[bits]
                blocks = cdiv(ncols, 64 * cols)
                cases.append(dict(form=form, cell=cell, bits=bits, vb=vb, mt=mt, m=m, kdim=kdim, ncols=ncols, k=k, oob=k < (1 << bits),
                                  wide=wname == "wide", mode="direct" if blocks == 1 else "split", id=f"b{bits}-vb{vb}-mt{mt}-m{m}-kd{kdim}-{wname}",
                                  expect=dict(col_tiles=blocks, splits=blocks)))
                if form == "gpacked_bwd":
                    cases[-1]["group_rows"] = group_rows_for(kdim)
                    cases[-1]["expect"]["groups"] = cdiv(kdim, group_rows_for(kdim))
                    assert cases[-1]["expect"]["groups"] == 3 and kdim % group_rows_for(kdim)
    return cases


CASES = {"byte": _dense_cases("byte"), "sparse": _sparse_cases(), "grouped": _dense_cases("grouped"), "packed": _packed_cases("packed"),
         "gpacked": _packed_cases("gpacked"), "packed_bwd": _packed_bwd_cases("packed_bwd"), "gpacked_bwd": _packed_bwd_cases("gpacked_bwd")}
BY_ID = {form: {c["id"]: c for c in cases} for form, cases in CASES.items()}


def cell_of_plan(case, plan):
    """The cell a plan of the case's unit reports (the label width and the bits are the call's own arguments)."""
    form = case["form"]
    if form == "byte":
        return (case["lb"], plan["vb"], plan["mt"], plan["aligned"])
    if form == "sparse":
        return (case["lb"], plan["mt"])
    if form == "grouped":
        return (plan["vb"], plan["mt"], plan["aligned"])
    return (case["bits"], plan["vb"], plan["mt"])


def labels_addr(case, base=256):
    return base + case.get("off", 0) * case.get("lb", 1)


def _tdt(dtype):
    import torch

    return {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[dtype]


def plan(case, dtype, cus, addr=None, one_group=False):
    """(plan, workspace bytes) of the case's forward unit for ``dtype`` on ``cus`` compute units; ``one_group``: of nnc_cbpk_h16, the
    grouped packed unit with one group.  Host only."""
    from neural_network_compression_amd import _native as nat
    from neural_network_compression_amd import ops

    lib = nat.load()
    form, m, kdim, ncols, k = case["form"], case["m"], case["kdim"], case["ncols"], case["k"]
    code = {"f32": 0, "bf16": 1, "fp16": 2}[dtype]
    addr = labels_addr(case) if addr is None else addr
    if form == "byte":
        return (ops.cbmm_h16_plan(_tdt(dtype), m, kdim, ncols, case["lb"], k, cus, addr), int(lib.nnc_cbmm_h16_workspace_bytes(m, kdim, ncols, case["lb"])))
    if form == "sparse":
        return (ops.cbsp_h16_plan(_tdt(dtype), m, kdim, ncols, case["lb"], k, cus), int(lib.nnc_cbsp_h16_workspace_bytes(m, kdim, ncols, case["lb"])))
    if form == "grouped":
        return (ops.cbmm_grouped_plan(_tdt(dtype), m, kdim, ncols, k, case["group_rows"], cus, addr),
                int(lib.nnc_cbmm_grouped_workspace_bytes(code, m, kdim, ncols)))
    if form == "packed":
        return (ops.cbpk_plan(m, kdim, ncols, case["bits"], k, cus), int(lib.nnc_cbpk_workspace_bytes(m, kdim, ncols, case["bits"])))
    assert form == "gpacked", form
    if one_group:
        return (ops.cbpk_h16_plan(_tdt(dtype), m, kdim, ncols, case["bits"], k, cus), int(lib.nnc_cbpk_h16_workspace_bytes(m, kdim, ncols, case["bits"])))
    return (ops.cbpk_grouped_plan(_tdt(dtype), m, kdim, ncols, case["bits"], k, case["group_rows"], cus),
            int(lib.nnc_cbpk_grouped_workspace_bytes(code, m, kdim, ncols, case["bits"])))


def bwd_plans(case, dtype, cus):
    """(dx plan, dc plan, dx workspace bytes, dc workspace bytes) of nnc_cbpk_dx_h16 / nnc_cbpk_dc_h16, or of nnc_cbpk_grouped_dx_h16 /
    nnc_cbpk_grouped_dc_h16 for the grouped form"""
    from neural_network_compression_amd import _native as nat
    from neural_network_compression_amd import ops

    lib = nat.load()
    a = (case["m"], case["kdim"], case["ncols"], case["bits"])
    if case["form"] == "gpacked_bwd":
        b = (*a, case["k"], case["group_rows"])
        return (ops.cbpk_grouped_dx_h16_plan(_tdt(dtype), *b, cus), ops.cbpk_grouped_dc_h16_plan(_tdt(dtype), *b, cus),
                int(lib.nnc_cbpk_grouped_dx_h16_workspace_bytes(*a)), int(lib.nnc_cbpk_grouped_dc_h16_workspace_bytes(*b)))
    return (ops.cbpk_dx_h16_plan(_tdt(dtype), *a, case["k"], cus), ops.cbpk_dc_h16_plan(_tdt(dtype), *a, case["k"], cus),
            int(lib.nnc_cbpk_dx_h16_workspace_bytes(*a)), int(lib.nnc_cbpk_dc_h16_workspace_bytes(*a, case["k"])))


def check_plan(case, p, cus, one_group=False):
    """Assert that the forward plan ``p`` at ``cus`` compute units is what the case claims; -> the cell it reports."""
    what = (case["id"], cus, p)
    assert p["path"] == PATH_STREAM, what
    assert cell_of_plan(case, p) == case["cell"], what
    assert p["mt"] >= case["m"] > p["mt"] // 2, what
    splits, rps = split_of(case, cus)
    assert (p["col_tiles"], p["splits"], p["rps"]) == (case["expect"]["col_tiles"], splits, rps), (what, splits, rps)
    if case["mode"] == "direct":
        assert splits == 1, what
    else:
        assert splits >= 2 and case["kdim"] % rps, what                   # a ragged last split
    if "group_rows" in case and not one_group:
        assert (p["group_rows"], p["groups"]) == (case["group_rows"], case["expect"]["groups"]), what
        assert p["max_groups_per_split"] == groups_in_a_split(case, cus), what
    return cell_of_plan(case, p)


# ------------------------------------------------------------------ data and references
def pack(lab, bits):
    """packed_ref.pack of (kdim, ncols) labels below 2^bits, without its loop over the columns -> uint8[kdim * row_bytes]"""
    kdim, ncols = lab.shape
    per, rb = 8 // bits, packed_ref.row_bytes(ncols, bits)
    full = np.zeros((kdim, rb * per), dtype=np.uint8)
    full[:, :ncols] = lab
    full = full.reshape(kdim, rb, per)
    out = np.zeros((kdim, rb), dtype=np.uint8)
    for j in range(per):
        out |= full[:, :, j] << np.uint8(bits * j)
    return out.reshape(-1)


def _seed(case):
    return 1 + CASES[case["form"]].index(BY_ID[case["form"]][case["id"]])


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _centres(rng, shape):
    return (rng.randint(-8, 9, size=shape) / 4.0).astype(np.float32)


def _offsets(step, groups, k):
    """group q's centres are offset by +- step q (the sign alternates with the index, so that a pre-activation takes both signs): a row
    read from another group's table is off by ``step`` or more per unit of x"""
    return (step * np.arange(groups, dtype=np.float32)[:, None] * np.where(np.arange(k) % 2, -1.0, 1.0)[None, :]).astype(np.float32)


def _product(x, table_rows, lab, chunk=1 << 22):
    """(x @ W, |x| @ |W|) in float64, W[i, o] = table_rows[i][lab[i, o]] never held whole: column chunks of about ``chunk`` weights"""
    kdim, ncols = lab.shape
    x64 = x.astype(np.float64)
    y, mag = np.empty((x.shape[0], ncols)), np.empty((x.shape[0], ncols))
    step = max(1, chunk // kdim)
    rows = np.arange(kdim)[:, None]
    for c0 in range(0, ncols, step):
        w = table_rows[rows, lab[:, c0: c0 + step]].astype(np.float64)
        y[:, c0: c0 + step] = x64 @ w
        mag[:, c0: c0 + step] = np.abs(x64) @ np.abs(w)
    return y, mag


def _finish(case, y, mag, bias):
    """+ bias, ReLU; the precondition of bit for bit; with ReLU on, pre-activations of both signs"""
    if bias is not None:
        y, mag = y + bias.astype(np.float64), mag + np.abs(bias).astype(np.float64)
    if case["relu"]:
        assert (y < 0).any() and (y > 0).any(), case["id"]
        y = np.where(y < 0, 0.0, y)
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y)
    return y, assert_exact(mag)


@functools.lru_cache(maxsize=None)
def _packed_shape(bits, kdim, ncols, k, seed):
    """What the cases of one wide shape share: the labels (uint8), their packed bytes, the centres of three groups"""
    rng = np.random.RandomState(seed)
    lab = rng.randint(0, 1 << bits, size=(kdim, ncols)).astype(np.uint8)
    if k == 1 << bits:
        assert lab.max() < k
    cen = _centres(rng, (cdiv(kdim, group_rows_for(kdim)), k)) + _offsets(16.0, cdiv(kdim, group_rows_for(kdim)), k)
    for dtype in ("bf16", "fp16"):
        assert np.array_equal(round_to(cen, dtype).reshape(cen.shape), cen)        # the kernels' rounding is the identity
    return lab, pack(lab, bits), cen


@functools.lru_cache(maxsize=None)
def _data(form, case_id, dtype):
    case = BY_ID[form][case_id]
    m, kdim, ncols, k = case["m"], case["kdim"], case["ncols"], case["k"]
    rng = np.random.RandomState(_seed(case))
    x = rng.randint(-3, 4, size=(m, kdim)).astype(np.float32)
    bias = rng.randint(-50, 51, size=ncols).astype(np.float32) if case.get("bias") else None
    rnd = (lambda c: c) if dtype == "f32" else (lambda c: round_to(c, dtype).reshape(c.shape))
    out = dict(x=x, bias=bias)
    if form in ("byte", "grouped"):
        groups = cdiv(kdim, case["group_rows"]) if form == "grouped" else 1
        cen = _centres(rng, (groups, k)) + (_offsets(64.0, groups, k) if form == "grouped" else 0)
        lab = rng.randint(0, k, size=(kdim, ncols))
        if case["oob"]:
            past = rng.random_sample(lab.shape) < 0.05
            past[0, 0] = True
            lab[past] = rng.randint(k, 256 if case["lb"] == 1 else k + 50, size=int(past.sum()))
            assert (lab >= k).any()
        if form == "byte":
            assert np.array_equal(round_to(cen, "bf16").reshape(cen.shape), cen) and np.array_equal(round_to(cen, "fp16").reshape(cen.shape), cen)
        table = np.concatenate([rnd(cen), np.zeros((groups, 256 if case["lb"] == 1 else k + 50), dtype=np.float32)], axis=1)
        y, mag = _product(x, table[np.arange(kdim) // case.get("group_rows", kdim + 1)], lab)
        out.update(centers=cen if form == "grouped" else cen[0], labels=lab)
    elif form == "sparse":
        z = case["z"]
        cen = _centres(rng, k)
        cen[z] = 0.75
        assert np.array_equal(round_to(cen, "bf16"), cen) and np.array_equal(round_to(cen, "fp16"), cen)
        lab = labels_at_density(rng, kdim, ncols, k, SPARSE_DENSITY, z)
        if case["oob"]:
            stored = np.argwhere(lab != z)
            pick = stored[rng.choice(len(stored), size=max(1, len(stored) // 20), replace=False)]
            lab[pick[:, 0], pick[:, 1]] = rng.randint(k, 256 if case["lb"] == 1 else k + 50, size=len(pick))
            assert (lab >= k).any()
        assert 0 < (lab != z).sum() < lab.size
        table = np.concatenate([cen, np.zeros(256 if case["lb"] == 1 else 50, dtype=np.float32)])
        y, mag = _product(x, np.broadcast_to(table, (kdim, table.size)), lab)
        # the kernel sums c_z sum x + x @ (W - c_z): its partial sums are bounded by |x| @ (|W| + |c_z|) + |c_z| sum |x|
        mag = mag + 2 * 0.75 * np.abs(x).astype(np.float64).sum(axis=1, keepdims=True)
        out.update(centers=cen, labels=lab)
    else:
        bits = case["bits"]
        lab, packed, cen = _packed_shape(bits, kdim, ncols, k, 77 if case["wide"] else _seed(case))
        if case["oob"]:
            assert (lab >= k).any()
        table = np.concatenate([cen, np.zeros((cen.shape[0], 16), dtype=np.float32)], axis=1)
        out.update(packed=packed, centers=cen)
        if form == "gpacked":
            assert cen.shape[0] == case["expect"]["groups"]
            y, mag = _product(x, table[np.arange(kdim) // case["group_rows"]], lab)
        y1, mag1 = _product(x, np.broadcast_to(table[0], (kdim, table.shape[1])), lab)       # one group: the first row of centres
        out["y1"], top1 = _finish(case, y1, mag1, bias)
        if form == "packed":
            out.update(y=out["y1"], top=top1)
            return _frozen(out)
    out["y"], out["top"] = _finish(case, y, mag, bias)
    return _frozen(out)


def data(case, dtype):
    """dict(x, bias or None, centers, labels or packed, y[, y1], top): the inputs (read-only, shared) and the float64 result of the unit
    run with ``dtype``; y1: the result with the first group's centres throughout (nnc_cbpk_h16).  The packed forms compute one
    product for the three element types."""
    form = case["form"]
    return _data(form, case["id"], dtype if form == "grouped" else "f32")      # (elsewhere the kernels' rounding of the centres is the identity: asserted)


@functools.lru_cache(maxsize=None)
def bwd_data(form, case_id):
    """dict(x, g, centers, packed, dx, dc, top) of a packed backward case: integer x and g in [-3, 3], quarter-integer centres (exact in
    both half types; the grouped form's offset by +- 16 per group), the labels up to 2^bits - 1 where K is smaller; dx = g @ W^T and
    dc[q, j] = the sum of (x^T g)[i, o] over the (i, o) of group q with label j (a label >= K reads 0 and falls into no bin), float64,
    formed a block of rows at a time.  dc has the unit's shape: [K], or [G, K] for the grouped form."""
    from . import cbgrad_ref

    case = BY_ID[form][case_id]
    m, kdim, ncols, k, bits = case["m"], case["kdim"], case["ncols"], case["k"], case["bits"]
    gr = case.get("group_rows", kdim)
    G = cdiv(kdim, gr)
    rng = np.random.RandomState(_seed(case))
    x = rng.randint(-3, 4, size=(m, kdim)).astype(np.float32)
    g = rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
    lab, packed, _ = _packed_shape(bits, kdim, ncols, k, 78 if case["wide"] else 500 + _seed(case))
    cen = _centres(rng, (G, k)) + _offsets(16.0, G, k)
    cen[:, 0] += 0.75 - cen[0, 0]
    assert all(np.array_equal(round_to(cen, dt).reshape(cen.shape), cen) for dt in ("bf16", "fp16"))
    table = np.concatenate([cen, np.zeros((G, 16), dtype=np.float32)], axis=1)
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    dx, mag, dc = np.empty((m, kdim)), np.empty((m, kdim)), np.zeros(G * 16)
    step = max(1, (1 << 22) // ncols)
    for i0 in range(0, kdim, step):
        rows = np.arange(i0, min(kdim, i0 + step))
        li = lab[rows]
        w = table[(rows // gr)[:, None], li].astype(np.float64)
        dx[:, rows] = g64 @ w.T
        mag[:, rows] = np.abs(g64) @ np.abs(w).T
        dc += np.bincount(((rows // gr)[:, None] * 16 + li).ravel(), weights=(x64[:, rows].T @ g64).ravel(), minlength=G * 16)
    dc = dc.reshape(G, 16)[:, :k].copy()
    if form == "packed_bwd":
        cen, dc = cen[0], dc[0]
        if not case["wide"]:
            assert np.array_equal(dx, cbgrad_ref.dx64(g, lab.astype(np.int64), cen)) and np.array_equal(dc, cbgrad_ref.dc64(x, g, lab.astype(np.int64), k))
    top = assert_exact(mag, np.abs(x64).T @ np.abs(g64))
    return _frozen(dict(x=x, g=g, centers=cen, packed=packed, dx=dx, dc=dc, top=top))
