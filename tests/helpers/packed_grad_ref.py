"""References and the case list for the packed codebook backward tests (ops.packed_codebook_matmul_dx /
packed_codebook_centroid_grad / packed_codebook_linear, csrc/nnc_cbpkgrad.hip).

- ``dx64`` / ``dc64``: the float64 formulas of include/nnc.h on the labels the packed buffer holds (packed_ref.unpack of
  packed_ref.pack: a label >= K reads 0 in dx and falls into no bin in dc; the padding is not part of the matrix).
- ``dx_bound``: the DESIGN.md section 12 bound of |dx - g @ W^T| (W decoded, float64).  It is derived, not measured: a float32 sum
  of ncols products in any order stays inside it, so the packed kernel's column blocking needs no extra margin.
- ``CASES`` / ``dx_regime`` / ``dc_regime`` / ``cells``: calls that, between them, hit every regime of the two plans, every MT
  at both widths, K at and below 2^bits, rows that fill their 16-byte groups and rows that leave padding, kdim = 1 and ncols = 1.
Test infrastructure only."""
from __future__ import annotations

import itertools

import numpy as np

from tests.helpers import cbgrad_ref, packed_ref

U = 2.0 ** -24
PATH_NONE, PATH_STREAM, PATH_TILED, PATH_ZERO = 0, 1, 2, 4


def held_labels(lab, bits):
    """The (kdim, ncols) labels as the packed buffer holds them: through the NumPy pack and unpack of the layout."""
    lab = np.asarray(lab)
    kdim, ncols = lab.shape
    return packed_ref.unpack(packed_ref.pack(lab, kdim, ncols, bits), kdim, ncols, bits).reshape(kdim, ncols).astype(np.int64)


def dx64(g, lab, centers, bits):
    return cbgrad_ref.dx64(g, held_labels(lab, bits), centers)


def dc64(x, g, lab, k, bits):
    return cbgrad_ref.dc64(x, g, held_labels(lab, bits), k)


def dx_bound(g, lab, centers):
    """(g @ W^T in float64, 2 (ncols + 4) u (|g| |W|^T))."""
    return cbgrad_ref.dx64(g, lab, centers), cbgrad_ref.dx_bound(g, lab, centers) + 1e-30


# ------------------------------------------------------------------ the regime matrix
# name, m, kdim, ncols, bits, K.  The labels are drawn up to 2^bits - 1, so with K < 2^bits labels >= K occur.
CASES = [
    ("stream_m1_b4_k16_oneblock", 1, 37, 200, 4, 16),
    ("stream_m1_b2_k3_oneblock_n1", 1, 50, 1, 2, 3),
    ("stream_m1_b4_k5_blocks", 1, 300, 5000, 4, 5),
    ("stream_m1_b2_k4_blocks", 1, 129, 9000, 2, 4),
    ("stream_m2_b4_k1_n33", 2, 65, 33, 4, 1),
    ("stream_m2_b2_k1_kdim1_n64", 2, 1, 64, 2, 1),
    ("stream_m3_b4_k16_blocks_n1040", 3, 70, 1040, 4, 16),
    ("stream_m4_b2_k3_blocks_n1027", 4, 96, 1027, 2, 3),
    ("stream_m5_b4_k5_n31", 5, 40, 31, 4, 5),
    ("stream_m7_b2_k4_blocks", 7, 200, 700, 2, 4),
    ("stream_m8_b4_k16_blocks_n1027", 8, 33, 1027, 4, 16),
    ("stream_m12_b4_k1_kdim1_n7", 12, 1, 7, 4, 1),
    ("stream_m16_b4_k16_blocks", 16, 90, 600, 4, 16),
    ("stream_m16_b2_k4_oneblock_n50", 16, 77, 50, 2, 4),
    ("stream_m16_b2_k3_blocks", 16, 64, 333, 2, 3),
    ("stream_m9_b4_k5_oneblock_n32", 9, 20, 32, 4, 5),
    ("stream_m6_b2_k1_n7", 6, 31, 7, 2, 1),
    ("tiled_m17_b4_k16_nosplit", 17, 100, 100, 4, 16),
    ("tiled_m17_b2_k3_nosplit_n1", 17, 50, 1, 2, 3),
    ("tiled_m40_b4_k5_split", 40, 100, 300, 4, 5),
    ("tiled_m40_b2_k4_split_n1027", 40, 60, 1027, 2, 4),
    ("tiled_m200_b4_k1_kdim1_split", 200, 1, 513, 4, 1),
    ("tiled_m256_b2_k4_msplit", 256, 100, 70, 2, 4),
    ("tiled_m300_b4_k16_msplit_n33", 300, 33, 33, 4, 16),
    ("tiled_m300_b2_k1_msplit", 300, 40, 129, 2, 1),
    ("empty_m", 0, 50, 60, 4, 8),
    ("empty_kdim", 4, 0, 60, 2, 3),
    ("empty_ncols", 4, 50, 0, 4, 16),
    ("empty_ncols_tiled", 20, 50, 0, 2, 4),
]


def regime(plan):
    p = plan["path"]
    return (p, plan["splits"] > 1) if p in (PATH_STREAM, PATH_TILED) else (p, False)


DX_REQUIRED = {(PATH_STREAM, False), (PATH_STREAM, True), (PATH_TILED, False), (PATH_TILED, True), (PATH_NONE, False), (PATH_ZERO, False)}
DC_REQUIRED = {(PATH_STREAM, False), (PATH_TILED, False), (PATH_TILED, True), (PATH_ZERO, False)}


def cells(case, dxp, dcp):
    """What a case contributes besides its two regimes: (mt, bits) of a stream call, (K, bits), the row fill, kdim = 1, ncols = 1."""
    _, m, kdim, ncols, bits, k = case
    out = {("k", bits, k)}
    if m * kdim * ncols:
        out.add(("row", bits, "exact" if ncols * bits % 128 == 0 else "padded"))
        if ncols in packed_ref.NCOLS:
            out.add(("ncols", ncols))
        if kdim == 1:
            out.add(("kdim", 1))
    if dxp["path"] == PATH_STREAM:
        assert dcp["path"] == PATH_STREAM and (dxp["mt"], dxp["vb"]) == (dcp["mt"], dcp["vb"])
        out.add(("mt", bits, dxp["mt"]))
    return out


def required_cells():
    req = {("mt", bits, mt) for bits, mt in itertools.product(packed_ref.BITS, packed_ref.MTS)}
    req |= {("k", bits, k) for bits in packed_ref.BITS for k in packed_ref.KS[bits]}
    req |= {("row", bits, fill) for bits in packed_ref.BITS for fill in ("exact", "padded")}
    req |= {("ncols", n) for n in packed_ref.NCOLS} | {("kdim", 1)}
    return req


def coverage(ops, cus):
    """(dx regimes, dc regimes, cells) the case list reaches on a device of ``cus`` compute units."""
    dxs, dcs, cs = set(), set(), set()
    for case in CASES:
        _, m, kdim, ncols, bits, k = case
        dxp, dcp = ops.cbpk_dx_plan(m, kdim, ncols, bits, k, cus), ops.cbpk_dc_plan(m, kdim, ncols, bits, k, cus)
        dxs.add(regime(dxp))
        dcs.add(regime(dcp))
        cs |= cells(case, dxp, dcp)
    return dxs, dcs, cs


def assert_covered(ops, cus):
    dxs, dcs, cs = coverage(ops, cus)
    assert DX_REQUIRED <= dxs and DC_REQUIRED <= dcs, (cus, DX_REQUIRED - dxs, DC_REQUIRED - dcs)
    assert required_cells() <= cs, (cus, required_cells() - cs)


def case_data(case, seed):
    """Exact data: integer x, g in [-3, 3], dyadic centres (multiples of 1/4 in [-2, 2], c[0] never 0), labels in [0, 2^bits)."""
    _, m, kdim, ncols, bits, k = case
    rng = np.random.RandomState(seed)
    x = rng.randint(-3, 4, size=(m, kdim)).astype(np.float32)
    g = rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
    c = (rng.randint(-8, 9, size=k) / 4.0).astype(np.float32)
    c[0] = 0.75
    lab = rng.randint(0, 1 << bits, size=(kdim, ncols))
    return x, g, c, lab
