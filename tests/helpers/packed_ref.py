"""The NumPy reference of the 2- and 4-bit packed index form and the case list of its tests (ops.pack_codes /
ops.packed_codebook_matmul, csrc/nnc_cbpk.hip, include/nnc.h nnc_cbpk_*).

- ``row_bytes`` / ``pack`` / ``unpack``: the layout as include/nnc.h states it, written from that text alone: rows of
  16 * ceil(ncols * bits / 128) bytes, label (i, o) in byte i * row_bytes + o * bits // 8 at bit o * bits % 8, padding 0.
- ``PACKED_REGIME_CASES`` / ``regime_of`` / ``required_regimes``: calls that, between them, hit every regime the plan
  (nnc_cbpk_plan) can choose, every K at and below 2^bits, rows that fill their 16-byte groups and rows that leave padding, and x
  and bias as plain tensors and as misaligned views; the CPU suite checks the coverage at several CU counts, the GPU suite at
  the device's own and runs every case.
Test infrastructure only."""
from __future__ import annotations

import itertools

import numpy as np

BITS = (2, 4)
MTS = (1, 2, 4, 8, 16)
KS = {2: (1, 3, 4), 4: (1, 5, 16)}                       # K at and below 2^bits
NCOLS = (1, 7, 31, 32, 33, 50, 64, 1027, 1040)           # 32 fills a 4-bit row, 64 a 2-bit and a 4-bit one; the others leave padding
PLAN_CUS = (1, 8, 104, 256, 304)


# ------------------------------------------------------------------ the layout
def row_bytes(ncols: int, bits: int) -> int:
    return 16 * (-(-(ncols * bits) // 128))


def pack(labels, kdim: int, ncols: int, bits: int) -> np.ndarray:
    """labels (kdim * ncols, each < 2^bits) -> uint8[kdim * row_bytes]."""
    lab = np.asarray(labels).reshape(kdim, ncols).astype(np.int64)
    assert lab.size == 0 or (lab.min() >= 0 and lab.max() < (1 << bits))
    out = np.zeros((kdim, row_bytes(ncols, bits)), dtype=np.uint8)
    for o in range(ncols):
        out[:, o * bits // 8] |= (lab[:, o] << (o * bits % 8)).astype(np.uint8)
    return out.reshape(-1)


def unpack(packed, kdim: int, ncols: int, bits: int) -> np.ndarray:
    """uint8[kdim * row_bytes] -> uint8[kdim * ncols]."""
    buf = np.asarray(packed, dtype=np.uint8).reshape(kdim, row_bytes(ncols, bits))
    out = np.zeros((kdim, ncols), dtype=np.uint8)
    for o in range(ncols):
        out[:, o] = (buf[:, o * bits // 8] >> (o * bits % 8)) & ((1 << bits) - 1)
    return out.reshape(-1)


# ------------------------------------------------------------------ the regime matrix
def regime_of(case, plan):
    """The cells of the matrix a call falls in (a set of tuples)."""
    bits = case["bits"]
    mode = "split" if plan["splits"] > 1 else "direct"
    fill = "exact" if case["ncols"] * bits % 128 == 0 else "padded"
    cells = {("k", bits, case["k"]), ("row", bits, fill),
             ("x", "view" if case["x_view"] else "plain"),
             ("bias", "none" if not case["bias"] else ("view" if case["bias_view"] else "plain"))}
    if case["ncols"] in NCOLS:
        cells.add(("ncols", case["ncols"]))
    if plan["path"] == 1:
        cells.add(("stream", bits, plan["mt"], mode))
    else:
        assert plan["path"] == 2, plan
        cells.add(("tiled", bits, mode))
    return cells


def required_regimes():
    req = {("stream", bits, mt, mode) for bits, mt, mode in itertools.product(BITS, MTS, ("direct", "split"))}
    req |= {("tiled", bits, mode) for bits, mode in itertools.product(BITS, ("direct", "split"))}
    req |= {("k", bits, k) for bits in BITS for k in KS[bits]}
    req |= {("ncols", n) for n in NCOLS}
    req |= {("row", bits, fill) for bits in BITS for fill in ("exact", "padded")}
    req |= {("x", v) for v in ("view", "plain")} | {("bias", v) for v in ("none", "view", "plain")}
    return req


def _regime_cases():
    """Every m in 1..16 at both widths, direct (kdim < 32: no wave keeps a full batch of rows, some none at all) and split (one
    column tile and kdim >= 64 m / bits, so that even one CU takes two splits); then m = 17..130 through the tiled kernel, direct
    (kdim < 256) and split.  K, ncols, and x / bias as views (buf[1:]) rotate through their lists."""
    cases = []
    direct_kdims = (1, 2, 3, 31, 17, 5, 20)
    split_kdims = (600, 777, 1000)
    split_ncols = (1, 7, 31, 32, 33, 50, 64)              # one column tile at every mt (64 lanes x 4 columns at mt = 16)
    i = 0
    for bits in BITS:
        for m in range(1, 17):
            for mode in ("direct", "split"):
                k = KS[bits][i % 3]
                kdim = direct_kdims[i % len(direct_kdims)] if mode == "direct" else split_kdims[i % len(split_kdims)]
                ncols = NCOLS[i % len(NCOLS)] if mode == "direct" else split_ncols[i % len(split_ncols)]
                cases.append(dict(m=m, kdim=kdim, ncols=ncols, bits=bits, k=k, x_view=i % 2 == 1, bias=i % 3 != 2, bias_view=i % 4 == 1,
                                  want=mode))
                i += 1
    for bits in BITS:
        for j, k in enumerate(KS[bits]):
            cases.append(dict(m=17, kdim=3, ncols=50, bits=bits, k=k, x_view=True, bias=True, bias_view=True, want="direct"))
            cases.append(dict(m=40, kdim=100, ncols=(129, 1027, 64)[j], bits=bits, k=k, x_view=False, bias=False, bias_view=False, want="direct"))
            cases.append(dict(m=17, kdim=300, ncols=(50, 32, 128)[j], bits=bits, k=k, x_view=False, bias=True, bias_view=False, want="split"))
            cases.append(dict(m=130, kdim=1001, ncols=(200, 33, 1)[j], bits=bits, k=k, x_view=True, bias=True, bias_view=True, want=None))   # four tiles: one CU does not split them
    return cases


PACKED_REGIME_CASES = _regime_cases()


def case_id(c):
    return f"m{c['m']}-kd{c['kdim']}-n{c['ncols']}-b{c['bits']}-k{c['k']}"
