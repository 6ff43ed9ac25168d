"""The MFMA tile instantiations of the fifteen half-precision codebook units (m > 16: five forward, five dx and five dc kernels over
csrc/nnc_cbmfma.hpp and dcm_accumulate of csrc/nnc_cbgrad_h16.hpp), and one case list per (form, direction) that reaches every one of
them in both modes, shared by tests/test_mfma_cells_abi.py (CPU: the tables against the sources, the plans, the
edges every cell sees, the cells the older lists reach) and tests/test_gpu_zzz_mfma_cells.py.

A *cell* is (form, direction, element type, form argument, XVEC arm, mode):

- form / direction: ``UNITS``; forward: byte, sparse, gbyte, gpacked (nnc_cbpk_h16 is that unit with one group), gsparse; dx and dc:
  byte, sparse, packed, gbyte, gpacked.
- form argument: the label bytes (1, 2) of the byte and sparse forms, the bits (4, 2) of the packed forms, None for gbyte / gsparse.
- arm: every kernel is compiled for XVEC true ("vec") and false ("elem"), chosen at launch (``arm_of``, the rule of hm_launch and
  dcm_xvec restated once): forward: x 16-byte aligned and kdim % 8 == 0; dx: g 16-byte aligned and ncols % 8 == 0; dc: x and g 4-byte
  aligned, kdim and ncols even.
- mode: "direct" (one split: the kernel stores the result itself) or "split" (float32 partials and a reduce; dc: int64 bins either way).

``TABLES`` holds the instantiations, 104 in all (forward 32, dx 36, dc 36), so 208 cells.  ``CASES[(form, direction)]`` holds the cases;
every case runs with both element types.  The shapes (R rows and C columns of output tiles, E the reduced extent; forward: m, ncols,
kdim; dx: m, kdim, ncols; dc: kdim, ncols, m):

- E: 56 (vec, direct: one k step and a tail of 24 whose last 16-byte fragment lies wholly past k_hi), 61 (elem, direct: a tail of 29);
  split: ``split_extent``, the first multiple of 8 from 128 on with two splits or more at 80, 256 and 304 CUs whose last split is ragged
  and holds a whole step and a tail (136: per_split 96, the last split 40), and the first extent behind it that is 5 past a multiple of
  8, as 61 is (141: a last split of 45).  For dc the arm does not depend on E = m, so both values of a mode alternate.
- the elem arm is reached by width (the extent one of the above; dc: kdim or ncols odd) and by address (a vec-eligible shape with x,
  or g, one element into its buffer); ``how`` says which.
- R: 17 (one tile, most rows empty) and 161 (two tiles, the second ragged across the 32-row accumulator boundary); C: 33 (one tile that
  reaches the second accumulator of one wave only) and 193 (two tiles, the second of 65 columns: one wave owns a single column).  dc:
  R and C from {33, 193}, + 1 where the arm needs them even (an elem cell of dc sees kdim 33 and 193 odd, ncols 33 and 193 odd, and
  34 / 194 with x, or g, one element in).  The pairs rotate, so every cell sees every value, not the product.
- grouped forms: six slots per cell with group_rows 32, 32, 64, 96, 128 and 224 (>= kdim): 4, 2, 2 (the boundary off the tile grid), 1
  and 1 tables per 128-row tile of dx / dc (``grouped_h16_grad_ref.tile_tables``), a last group shorter than 32 rows, and for the
  forward, whose table refills at a k step, a split that begins inside a group (per_split 96, group_rows 64: asserted from the plan).
- K = 200 (uint8) / 300 (uint16), 16 for gbyte / gsparse; the elem cases hold 5 % indices >= K.  The first case of every uint8 cell has
  K = 256 with centre 255 NaN and used by no label: the bytes behind the labels are 0xFF, so a label read past the buffer, or looked
  up past k_hi, reaches the result as NaN.  Packed: K alternates 2^bits and 5 / 3; every width leaves padding fields in the last
  16-byte group.  Sparse: density 0.3, the skipped symbol 5 with centre 0.75 (gsparse: symbol 5 + q, centre 0.75), one bitmap word
  all zero and one all set in every case; 193 columns put a single bit into the last word of a row.
- the epilogue rotates per (cell, slot): bias on / off, ReLU on / off (pre-activations of both signs: asserted); a case runs with the
  result as float32 and as the half type.

``data(case)``: integer x and g in [-3, 3], quarter-integer centres in [-2, 2], a grouped form's offset by +- 4 q (exact in bf16 and
fp16: asserted, so one float64 reference serves both element types), integer bias; the float64 results.  The precondition of "bit for
bit" is asserted there (``stream_cells_ref.assert_exact``).  Test infrastructure only."""
from __future__ import annotations

import functools

import numpy as np

from . import forward_stream_cells_ref as fcells
from . import grouped_h16_grad_ref, sparse_ref
from .h16_ref import DTYPES, PATH_MFMA, round_to, torch_dtype
from .sparse_ref import labels_at_density
from .stream_cells_ref import assert_exact

CU_COUNTS = fcells.CU_COUNTS
PLAN_CUS = fcells.PLAN_CUS
cdiv = fcells.cdiv
HM_TILE, HM_BK = 128, 32
DIRECTIONS = ("fwd", "dx", "dc")

# ------------------------------------------------------------------ the tables of instantiations
# (form, direction) -> (source, kernel, form arguments); every kernel x {bf16, fp16} x argument x {vec, elem}
UNITS = {
    ("byte", "fwd"): ("nnc_cbmm_h16.hip", "k_cbmm_mfma", (1, 2)),
    ("sparse", "fwd"): ("nnc_cbsp_h16.hip", "k_cbsp_mfma", (1, 2)),
    ("gbyte", "fwd"): ("nnc_cbmm_grouped.hip", "k_cbmm_mfma_grouped", (None,)),
    ("gpacked", "fwd"): ("nnc_cbpk_grouped.hip", "k_cbpk_mfma_grouped", (4, 2)),
    ("gsparse", "fwd"): ("nnc_cbsp_grouped_h16.hip", "k_cbspg_mfma", (None,)),
    ("byte", "dx"): ("nnc_cbgrad_h16.hip", "k_cbdx_mfma", (1, 2)),
    ("sparse", "dx"): ("nnc_cbspgrad_h16.hip", "k_cbspdx_mfma", (1, 2)),
    ("packed", "dx"): ("nnc_cbpk_h16.hip", "k_cbpkdx_mfma", (4, 2)),
    ("gbyte", "dx"): ("nnc_cbgrad_grouped_h16.hip", "k_cbdx_mfma_grouped", (None,)),
    ("gpacked", "dx"): ("nnc_cbpkgrad_grouped_h16.hip", "k_cbpkdx_mfma_grouped", (4, 2)),
    ("byte", "dc"): ("nnc_cbgrad_h16.hip", "k_cbdc_mfma", (1, 2)),
    ("sparse", "dc"): ("nnc_cbspgrad_h16.hip", "k_cbspdc_mfma", (1, 2)),
    ("packed", "dc"): ("nnc_cbpk_h16.hip", "k_cbpkdc_mfma", (4, 2)),
    ("gbyte", "dc"): ("nnc_cbgrad_grouped_h16.hip", "k_cbdc_mfma_grouped", (None,)),
    ("gpacked", "dc"): ("nnc_cbpkgrad_grouped_h16.hip", "k_cbpkdc_mfma_grouped", (4, 2)),
}
ARMS, MODES = ("vec", "elem"), ("direct", "split")
TABLES = {unit: tuple((dt, a, arm) for dt in DTYPES for a in args for arm in ARMS) for unit, (_, _, args) in UNITS.items()}
CELLS = {unit: frozenset((dt, a, arm, mode) for dt, a, arm in table for mode in MODES) for unit, table in TABLES.items()}
GROUPED = ("gbyte", "gpacked", "gsparse")


def arm_of(direction, x_addr, g_addr, kdim, ncols):
    """The XVEC arm a launch takes: hm_launch (forward: x and kdim; dx: g and ncols) and dcm_xvec"""
    if direction == "fwd":
        return "vec" if x_addr % 16 == 0 and kdim % 8 == 0 else "elem"
    if direction == "dx":
        return "vec" if g_addr % 16 == 0 and ncols % 8 == 0 else "elem"
    return "vec" if x_addr % 4 == 0 and g_addr % 4 == 0 and kdim % 2 == 0 and ncols % 2 == 0 else "elem"


def mfma_split(direction, tiles, extent, cus):
    """(splits, per_split) of the MFMA plans: two workgroups per CU (the forward plans for the device's CUs up to 256, the backward
    for 256 whatever the device), every split at least two k steps, 16 at the most, every split a whole number of steps"""
    cus = min(cus, PLAN_CUS) if direction == "fwd" else PLAN_CUS
    s = max(1, min(cdiv(2 * cus, tiles), extent // (2 * HM_BK), 16))
    per = cdiv(cdiv(extent, s), HM_BK) * HM_BK
    return cdiv(extent, per), per


DIRECT_EXTENT = {"vec": 56, "elem": 61}


def split_extent(arm):
    """vec: the first multiple of 8 from 128 on that every tile count of the cases (1, 2, 4) splits at every CU count, the last split
    ragged with a whole step and a tail; elem: the first extent behind it that is 5 past a multiple of 8"""
    start = HM_TILE if arm == "vec" else split_extent("vec") + 1
    for extent in range(start, start + 400):
        if extent % 8 != (0 if arm == "vec" else 5):
            continue
        got = [mfma_split(d, tiles, extent, cus) for d in ("fwd", "dx") for tiles in (1, 2, 4) for cus in CU_COUNTS]
        if all(s >= 2 and (extent - (s - 1) * per) > HM_BK and (extent - (s - 1) * per) % HM_BK for s, per in got):
            return extent
    raise AssertionError(arm)


SPLIT_EXTENT = {arm: split_extent(arm) for arm in ARMS}
EXTENT = {"direct": DIRECT_EXTENT, "split": SPLIT_EXTENT}
K_OF_LB = fcells.K_OF_LB
GROUPED_K, SMALL_K = 16, fcells.SMALL_K
SPARSE_Z, SPARSE_DENSITY, CZ = 5, 0.3, 0.75
BIG_GROUP = 224
# (R, C) of a plain form's slots, (R, C, group_rows) of a grouped form's; dc: rows and columns of dW, before the parity of the arm
PAIRS = ((17, 193), (161, 33))
DC_PAIRS = ((193, 33), (33, 193))
GROUP_SLOTS = ((17, 193, 32), (161, 33, 32), (17, 193, 64), (161, 193, 96), (17, 193, 128), (161, 33, BIG_GROUP))
DC_GROUP_SLOTS = ((193, 33, 32), (33, 193, 32), (193, 33, 64), (193, 193, 96), (193, 33, 128), (33, 193, BIG_GROUP))
ELEM_HOWS = {"fwd": ("width", "address"), "dx": ("width", "address"), "dc": ("width-k", "width-n", "address-x", "address-g")}


def _slots(form, direction, arm):
    """[(how, R, C, group_rows or None)] of one (argument, arm, mode)"""
    grouped = form in GROUPED
    base = ((DC_GROUP_SLOTS if direction == "dc" else GROUP_SLOTS) if grouped
            else tuple(p + (None,) for p in (DC_PAIRS if direction == "dc" else PAIRS)))
    hows = ("vec",) if arm == "vec" else ELEM_HOWS[direction]
    if direction == "dc" and arm == "elem":     # either width with the odd 33 and the odd 193: the pairs shift against the four hows
        order = (0, 1, 2, 3, 5, 4) if grouped else tuple((i + i // 4) % 2 for i in range(8))
        return [(hows[i % 4],) + base[j] for i, j in enumerate(order)]
    n = max(len(base), len(hows))
    return [(hows[i % len(hows)],) + base[i % len(base)] for i in range(n)]


def _tag(a, form):
    return "" if a is None else (f"u{8 * a}-" if form in ("byte", "sparse") else f"b{a}-")


def _cases(form, direction):
    cases = []
    for a in UNITS[(form, direction)][2]:
        for arm in ARMS:
            for mode in MODES:
                for i, (how, R, C, gr) in enumerate(_slots(form, direction, arm)):
                    xoff = goff = 0
                    if direction == "dc":
                        E = (EXTENT[mode]["vec"], EXTENT[mode]["elem"])[i % 2]
                        kdim, ncols, m = R + (how != "width-k"), C + (how != "width-n"), E
                        xoff, goff = int(how == "address-x"), int(how == "address-g")
                    else:
                        E = EXTENT[mode]["elem" if how == "width" else "vec"]
                        m, kdim, ncols = (R, E, C) if direction == "fwd" else (R, C, E)
                        xoff, goff = (int(how == "address"), 0) if direction == "fwd" else (0, int(how == "address"))
                    # bias with every other slot; ReLU with it in the direct cells and against it in the split ones: a cell sees both values of
                    # each, an (argument, arm) all four pairs
                    r = dict(bias=i % 2 == 0, relu=(i + (mode == "split")) % 2 == 0)
                    uint8 = form == "gbyte" or (form == "byte" and a == 1)
                    nan_centre = uint8 and i == 0
                    if form in ("byte", "sparse"):
                        k = 256 if nan_centre else K_OF_LB[a]
                    elif form in ("packed", "gpacked"):
                        k = (1 << a) if i % 2 == 0 else SMALL_K[a]
                    else:
                        k = 256 if nan_centre else GROUPED_K
                    c = dict(form=form, direction=direction, arg=a, arm=arm, how=how, mode=mode, m=m, kdim=kdim, ncols=ncols, xoff=xoff, goff=goff,
                             k=k, nan_centre=nan_centre, oob=arm == "elem" and not nan_centre and form not in ("packed", "gpacked"),
                             tiles=(cdiv(R if direction != "dc" else kdim, HM_TILE), cdiv(C if direction != "dc" else ncols, HM_TILE)), extent=E,
                             id=f"{form}-{direction}-{_tag(a, form)}{how}-{mode}-m{m}-kd{kdim}-n{ncols}" + (f"-r{gr}" if gr else ""), **r)
                    if gr:
                        c["group_rows"] = gr
                        c["groups"] = cdiv(kdim, gr)
                    if form in ("packed", "gpacked"):
                        assert ncols * a % 128                                   # padding fields in the last 16-byte group
                    cases.append(c)
    assert len({c["id"] for c in cases}) == len(cases)
    return cases


CASES = {unit: _cases(*unit) for unit in UNITS}
BY_ID = {unit: {c["id"]: c for c in cases} for unit, cases in CASES.items()}


def unit_of(case):
    return (case["form"], case["direction"])


def cells_of(case):
    """the two cells (one per element type) a case is built for"""
    return {(dt, case["arg"], case["arm"], case["mode"]) for dt in DTYPES}


def operand_addrs(case, base=256):
    """(x address, g address) of operands ``xoff`` / ``goff`` elements into 256-byte aligned buffers"""
    return base + 2 * case["xoff"], base + 2 * case["goff"]


def split_of(case, cus):
    return mfma_split(case["direction"], case["tiles"][0] * case["tiles"][1], case["extent"], cus)


def tile_tables(case):
    """the tables (dx) / sets of bins (dc) the fullest 128-row tile of a grouped backward case holds"""
    gr, kdim = case["group_rows"], case["kdim"]
    return max((min(kdim, lo + HM_TILE) - 1) // gr - lo // gr + 1 for lo in range(0, kdim, HM_TILE))


def second_split_opens_inside_a_group(case, cus):
    splits, per = split_of(case, cus)
    return splits >= 2 and per % case["group_rows"] != 0 and per < case["kdim"] and case["groups"] > 1


# ------------------------------------------------------------------ the plans
def plan(case, dtype, cus, one_group=False):
    """(plan, workspace bytes) of the case's entry point for ``dtype`` at ``cus`` compute units; ``one_group``: of nnc_cbpk_h16.  Host
    only.  (The MFMA plans do not depend on the labels' address.)"""
    from neural_network_compression_amd import _native as nat
    from neural_network_compression_amd import ops

    L = nat.load()
    form, d, a, m, kdim, ncols, k = case["form"], case["direction"], case["arg"], case["m"], case["kdim"], case["ncols"], case["k"]
    t, code, gr = torch_dtype(dtype), {"bf16": 1, "fp16": 2}[dtype], case.get("group_rows")
    if d == "fwd":
        if form == "byte":
            return ops.cbmm_h16_plan(t, m, kdim, ncols, a, k, cus), int(L.nnc_cbmm_h16_workspace_bytes(m, kdim, ncols, a))
        if form == "sparse":
            return ops.cbsp_h16_plan(t, m, kdim, ncols, a, k, cus), int(L.nnc_cbsp_h16_workspace_bytes(m, kdim, ncols, a))
        if form == "gbyte":
            return ops.cbmm_grouped_plan(t, m, kdim, ncols, k, gr, cus), int(L.nnc_cbmm_grouped_workspace_bytes(code, m, kdim, ncols))
        if form == "gsparse":
            return ops.cbsp_grouped_h16_plan(t, m, kdim, ncols, k, gr, cus), int(L.nnc_cbsp_grouped_h16_workspace_bytes(code, m, kdim, ncols))
        assert form == "gpacked"
        if one_group:
            return ops.cbpk_h16_plan(t, m, kdim, ncols, a, k, cus), int(L.nnc_cbpk_h16_workspace_bytes(m, kdim, ncols, a))
        return ops.cbpk_grouped_plan(t, m, kdim, ncols, a, k, gr, cus), int(L.nnc_cbpk_grouped_workspace_bytes(code, m, kdim, ncols, a))
    name = {"byte": "cbmm", "sparse": "cbsp", "packed": "cbpk", "gbyte": "cbmm_grouped", "gpacked": "cbpk_grouped"}[form]
    args = {"byte": (a, k), "sparse": (a, k), "packed": (a, k), "gbyte": (k, gr), "gpacked": (a, k, gr)}[form]
    p = getattr(ops, f"{name}_{d}_h16_plan")(t, m, kdim, ncols, *args, cus)
    ws_args = args if d == "dc" else (() if form == "gbyte" else (a,))          # dx: the label bytes or the bits; dc: the plan's own
    return p, int(getattr(L, f"nnc_{name}_{d}_h16_workspace_bytes")(m, kdim, ncols, *ws_args))


def check_plan(case, p, cus, one_group=False):
    """Assert that plan ``p`` at ``cus`` compute units is what the case claims: the MFMA path, the tiles, the splits and per_split of
    its mode, the groups; -> (splits, per_split)"""
    what = (case["id"], cus, p)
    assert p["path"] == PATH_MFMA and case["m"] > 16, what
    rt, ct = case["tiles"]
    splits, per = split_of(case, cus)
    assert (p["row_tiles"], p["col_tiles"], p["splits"], p["cps" if case["direction"] == "dx" else "rps"]) == (rt, ct, splits, per), (what, splits, per)
    last = case["extent"] - (splits - 1) * per
    if case["mode"] == "direct":
        assert splits == 1 and HM_BK < case["extent"] < 2 * HM_BK, what          # one whole k step and a tail
    else:
        assert splits >= 2 and case["extent"] % per and last > HM_BK and last % HM_BK, what   # a ragged last split: a whole step and a tail
    if case["arm"] == "vec" and case["direction"] != "dc":
        assert last % HM_BK <= HM_BK - 8, what                                    # the last 16-byte fragment of the tail lies wholly past k_hi
    if "group_rows" in case and not one_group:
        assert (p["group_rows"], p["groups"]) == (case["group_rows"], case["groups"]), what
        if case["direction"] == "fwd":
            assert p["max_groups_per_split"] == max((min(case["kdim"], lo + per) - 1) // case["group_rows"] - lo // case["group_rows"] + 1
                                                    for lo in range(0, case["kdim"], per)), what
        else:
            assert (p["max_groups_per_workgroup"], p["held"]) == (tile_tables(case), grouped_h16_grad_ref.tile_tables(case["group_rows"])), what
    return splits, per


# ------------------------------------------------------------------ data and references
def _seed(case):
    return 1 + CASES[unit_of(case)].index(BY_ID[unit_of(case)][case["id"]])


def zero_symbols(case):
    """the skipped symbol of every group of a gsparse case"""
    return np.array([(SPARSE_Z + q) % case["k"] for q in range(case["groups"])], dtype=np.uint8)


def _past_k(rng, lab, k, lb, keep=None):
    """5 % of the (kept) labels become indices >= K"""
    pick = (rng.random_sample(lab.shape) < 0.05) & (True if keep is None else keep)
    first = np.argwhere(np.ones(lab.shape, bool) if keep is None else keep)[0]
    pick[first[0], first[1]] = True
    lab[pick] = rng.randint(k, 256 if lb == 1 else k + 50, size=int(pick.sum()))
    assert (lab >= k).any()


def _sparse_words(rng, lab, z_of_row, k):
    """one bitmap word (64 columns of a row) all zero and one all set"""
    r0, r1 = 0, lab.shape[0] // 2
    lab[r0, :64] = z_of_row[r0]
    other = rng.randint(0, k - 1, size=lab[r1, :64].size)
    lab[r1, :64] = other + (other >= z_of_row[r1])


@functools.lru_cache(maxsize=None)
def _data(unit, case_id):
    case = BY_ID[unit][case_id]
    form, d, a, m, kdim, ncols, k = case["form"], case["direction"], case["arg"], case["m"], case["kdim"], case["ncols"], case["k"]
    gr = case.get("group_rows", kdim)
    G = cdiv(kdim, gr)
    rng = np.random.RandomState(_seed(case) + 1000 * DIRECTIONS.index(d))
    x = rng.randint(-3, 4, size=(m, kdim)).astype(np.float32)
    g = rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
    bias = rng.randint(-50, 51, size=ncols).astype(np.float32) if d == "fwd" and case["bias"] else None
    cen = fcells._centres(rng, (G, k)) + (fcells._offsets(4.0, G, k) if form in GROUPED else 0)
    row_group = np.arange(kdim) // gr
    lb = a if form in ("byte", "sparse") else 1
    out = dict(x=x, g=g, bias=bias)
    cz = 0.0
    if form in ("byte", "gbyte"):
        lab = rng.randint(0, 255 if case["nan_centre"] else k, size=(kdim, ncols))
        if case["oob"]:
            _past_k(rng, lab, k, lb)
    elif form in ("packed", "gpacked"):
        lab = rng.randint(0, 1 << a, size=(kdim, ncols))
        assert (lab >= k).any() == (k < (1 << a))
        out["packed"] = fcells.pack(lab.astype(np.uint8), a)
    else:
        zs = zero_symbols(case) if form == "gsparse" else np.full(G, SPARSE_Z)
        cen[np.arange(G), zs] = CZ
        cz = CZ
        lab = np.concatenate([labels_at_density(rng, min(kdim, (q + 1) * gr) - q * gr, ncols, k, SPARSE_DENSITY, int(zs[q])) for q in range(G)])
        _sparse_words(rng, lab, zs[row_group], k)
        keep = lab != zs[row_group][:, None]
        if case["oob"]:
            _past_k(rng, lab, k, lb, keep)
        bitmap = sparse_ref.pack_np(np.where(keep, 1, 0), kdim, ncols, 0)["bitmap"]
        full = [(1 << min(64, ncols - 64 * s)) - 1 for s in range(bitmap.shape[1])]
        assert (bitmap == 0).any() and any(int(bitmap[i, s]) == full[s] for i in range(kdim) for s in range(len(full))), case_id
        assert ncols != 193 or (bitmap[:, 3] <= 1).all()
        out["zs"] = zs.astype(np.uint8)
    if case["nan_centre"]:
        assert k == 256 and lab.max() < 255
        cen[:, 255] = np.nan
    finite = np.where(np.isnan(cen), 0.0, cen)
    assert all(np.array_equal(round_to(finite, dt).reshape(cen.shape), finite) for dt in DTYPES)      # the kernels' rounding is the identity
    table = np.concatenate([cen, np.zeros((G, 306), dtype=np.float32)], axis=1)
    W = table[row_group[:, None], lab].astype(np.float64)
    assert np.isfinite(W).all()
    out.update(centers=cen if form in GROUPED else cen[0], labels=lab)
    x64, g64, xa, ga = x.astype(np.float64), g.astype(np.float64), np.abs(x).astype(np.float64), np.abs(g).astype(np.float64)
    if d == "fwd":
        # (sparse: the kernel sums c_z sum x + x @ (W - c_z): bounded by |x| @ (|W| + |c_z|) + |c_z| sum |x|)
        out["y"], out["top"] = fcells._finish(case, x64 @ W, xa @ np.abs(W) + 2 * cz * xa.sum(axis=1, keepdims=True), bias)
        if form == "gpacked":
            W1 = table[0][lab].astype(np.float64)
            out["y1"], _ = fcells._finish(case, x64 @ W1, xa @ np.abs(W1), bias)
        return fcells._frozen(out)
    out["dx"] = g64 @ W.T
    valid = lab < k
    bins = np.bincount((row_group[:, None] * k + np.where(valid, lab, 0))[valid], weights=(x64.T @ g64)[valid], minlength=G * k).reshape(G, k)
    out["dc"] = bins if form in GROUPED else bins[0]
    out["top"] = assert_exact(ga @ np.abs(W).T + 2 * cz * ga.sum(axis=1, keepdims=True), xa.T @ ga)
    assert np.array_equal(out["dx"].astype(np.float32).astype(np.float64), out["dx"])
    return fcells._frozen(out)


def data(case):
    """dict(x, g, bias or None, centers, labels[, packed][, zs], then y[, y1] or dx and dc, top): the inputs (read-only, shared by both
    element types) and the float64 results; y1: with the first group's centres throughout (nnc_cbpk_h16); dc: [K], grouped [G, K]"""
    return _data(unit_of(case), case["id"])


# ------------------------------------------------------------------ the cells the older case lists reach
def _row(a, m, kdim, ncols, xoff, goff, *plan_args):
    return dict(arg=a, m=m, kdim=kdim, ncols=ncols, xoff=int(xoff), goff=int(goff), plan_args=plan_args)


def old_lists():
    """unit -> (the older hand-picked list(s) its GPU tests run, their cases as rows: the form argument, the shape, x and g at the start
    of a 256-byte aligned allocation or, as a buf[1:] view, one element in, and the arguments of the unit's plan call behind the shape)"""
    from neural_network_compression_amd import ops

    from . import (grouped_packed_ref, grouped_ref, grouped_sparse_h16_ref, h16_grad_ref, h16_ref, packed_h16_ref, sparse_h16_grad_ref,
                   sparse_h16_ref)

    gg = grouped_h16_grad_ref
    out = {
        ("byte", "fwd"): ("h16_ref.CASES", ops.cbmm_h16_plan,
                          [_row(c["lb"], c["m"], c["kdim"], c["ncols"], c["x_view"], 0, c["lb"], c["k"]) for c in h16_ref.CASES]),
        ("sparse", "fwd"): ("sparse_h16_ref.CASES", ops.cbsp_h16_plan,
                            [_row(c["lb"], c["m"], c["kdim"], c["ncols"], c["x_view"], 0, c["lb"], c["k"]) for c in sparse_h16_ref.CASES]),
        ("gbyte", "fwd"): ("grouped_ref.CASES", ops.cbmm_grouped_plan,
                           [_row(None, c["m"], c["kdim"], c["ncols"], c["x_view"], 0, c["k"], c["group_rows"]) for c in grouped_ref.CASES]),
        ("gpacked", "fwd"): ("grouped_packed_ref.CASES, packed_h16_ref.MFMA_FORWARD (one group)", ops.cbpk_grouped_plan,
                             [_row(c["bits"], c["m"], c["kdim"], c["ncols"], c["x_view"], 0, c["bits"], c["k"], c["group_rows"]) for c in grouped_packed_ref.CASES]
                             + [_row(c[4], c[1], c[2], c[3], v, 0, c[4], c[5], 32 * cdiv(c[2], 32)) for c, v in packed_h16_ref.MFMA_FORWARD]),
        ("gsparse", "fwd"): ("grouped_sparse_h16_ref.CASES", ops.cbsp_grouped_h16_plan,
                             [_row(None, c["m"], c["kdim"], c["ncols"], c["x_view"], 0, c["k"], c["group_rows"]) for c in grouped_sparse_h16_ref.CASES]),
    }
    for way in ("dx", "dc"):
        out[("byte", way)] = ("h16_grad_ref.FULL", getattr(ops, f"cbmm_{way}_h16_plan"), [_row(c[4], c[1], c[2], c[3], v, v, c[4], c[5]) for c, v in h16_grad_ref.FULL])
        out[("sparse", way)] = ("sparse_h16_grad_ref.CASES", getattr(ops, f"cbsp_{way}_h16_plan"),
                                [_row(c["lb"], c["m"], c["kdim"], c["ncols"], c["view"], c["view"], c["lb"], c["k"]) for c in sparse_h16_grad_ref.CASES])
        out[("packed", way)] = ("packed_h16_ref.FULL", getattr(ops, f"cbpk_{way}_h16_plan"), [_row(c[4], c[1], c[2], c[3], v, v, c[4], c[5]) for c, v in packed_h16_ref.FULL])
        out[("gbyte", way)] = ("grouped_h16_grad_ref.CASES", getattr(ops, f"cbmm_grouped_{way}_h16_plan"),
                               [_row(None, c["m"], c["kdim"], c["ncols"], c["view"], c["view"], c["k"], c["group_rows"]) for c in gg.CASES])
        out[("gpacked", way)] = ("grouped_h16_grad_ref.PACKED_CASES", getattr(ops, f"cbpk_grouped_{way}_h16_plan"),
                                 [_row(c["bits"], c["m"], c["kdim"], c["ncols"], c["view"], c["view"], c["bits"], c["k"], c["group_rows"]) for c in gg.PACKED_CASES])
    return out


def cells_reached(unit, plan_fn, rows, cus):
    """the cells of ``unit`` that ``rows`` reach at ``cus`` compute units: the plan call says MFMA and direct / split, ``arm_of`` the arm"""
    hit = set()
    for r in rows:
        if min(r["m"], r["kdim"], r["ncols"]) < 1:
            continue
        xa, ga = 256 + 2 * r["xoff"], 256 + 2 * r["goff"]
        for dt in DTYPES:
            p = plan_fn(torch_dtype(dt), r["m"], r["kdim"], r["ncols"], *r["plan_args"], cus)
            if p["path"] == PATH_MFMA:
                hit.add((dt, r["arg"], arm_of(unit[1], xa, ga, r["kdim"], r["ncols"]), "split" if p["splits"] > 1 else "direct"))
    assert hit <= CELLS[unit], (unit, hit - CELLS[unit])
    return hit
