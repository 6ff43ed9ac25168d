"""The case list of the half-precision packed codebook tests (nnc_cbpk_h16 / nnc_cbpk_dx_h16 / nnc_cbpk_dc_h16,
csrc/nnc_cbpk_h16.hip), shared by tests/test_packed_codebook_h16_abi.py (CPU: the plans) and the two GPU files.

- ``CASES``: the smallest shapes that still reach every cell {stream, MFMA} x {2, 4 bits} x {direct, split} x {bf16, fp16} of dx and
  of dc (every case runs with both dtypes; the dc stream plan never splits m), both ``XVEC`` arms of each MFMA kernel (the aligned
  m = 64 row and the ``buf[1:]`` views), K at and below 2^bits, labels beyond K, and the four empty shapes of
  ``cbgrad_ref.REGIME_CASES``.  A case is a ``cbgrad_ref`` tuple with the bits where the label bytes stand and labels below 2^bits
  (``case_data``), and a flag: x and g as ``buf[1:]`` views.
- ``MFMA_FORWARD``: the forward cases beyond ``packed_ref.PACKED_REGIME_CASES`` (which reach the split stream plans): the rows of
  ``CASES`` above 16 rows of x.
- ``regime_of`` / ``required_regimes``: the cell a plan lies in, and the cells the list has to hit.
Test infrastructure only."""
from __future__ import annotations

import itertools

import numpy as np

from . import cbgrad_ref
from .h16_ref import DTYPES, PATH_MFMA, PATH_STREAM

PATH_NONE, PATH_ZERO = cbgrad_ref.PATH_NONE, cbgrad_ref.PATH_ZERO

# (name, m, kdim, ncols, bits, K, 0, labels beyond K), x and g as buf[1:] views
CASES = [
    (("stream_m1_b4_k16", 1, 37, 208, 4, 16, 0, False), False),
    (("stream_m5_b2_k3_beyond", 5, 129, 700, 2, 3, 0, True), False),
    (("stream_m16_b4_k5_views", 16, 40, 1000, 4, 5, 0, False), True),
    (("stream_m2_kdim1_b2", 2, 1, 77, 2, 4, 0, False), False),
    (("stream_m9_b4_beyond", 9, 40, 300, 4, 16, 0, True), False),
    (("mfma_m17_b4_direct", 17, 100, 100, 4, 16, 0, False), False),
    (("mfma_m40_b2_dxsplit", 40, 100, 300, 2, 4, 0, False), False),
    (("mfma_m130_b4_msplit_beyond", 130, 33, 129, 4, 5, 0, True), False),
    (("mfma_m200_kdim1_b2_k1", 200, 1, 513, 2, 1, 0, False), False),
    (("mfma_m64_aligned_xvec", 64, 128, 136, 4, 16, 0, False), False),
    (("mfma_m256_b2_views", 256, 130, 70, 2, 3, 0, False), True),
    (("mfma_m300_b4_k1", 300, 33, 129, 4, 1, 0, False), False),
] + [((c[0], c[1], c[2], c[3], 2 + 2 * (i % 2), 2, 0, False), False) for i, c in enumerate(c for c in cbgrad_ref.REGIME_CASES if c[0].startswith("empty_"))]

FULL = [c for c in CASES if not c[0][0].startswith("empty_")]
MFMA_FORWARD = [c for c in FULL if c[0][1] > 16]


def case_id(c):
    return c[0][0]


def case_data(case, seed):
    """``cbgrad_ref.case_data``'s exact data (integer x, g in [-3, 3], dyadic centres) with labels below 2^bits: in [0, K), or,
    with labels beyond K, anywhere in [0, 2^bits) where K < 2^bits."""
    _, m, kdim, ncols, bits, k, _, beyond = case
    x, g, c, _ = cbgrad_ref.case_data((None, m, kdim, ncols, 1, k, 0, False), seed)
    rng = np.random.RandomState(1000 + seed)
    lab = rng.randint(0, (1 << bits) if beyond else k, size=(kdim, ncols))
    return x, g, c, lab


def regime_of(case, plan, dtype):
    """(path, bits, direct / split, dtype) of a dx or dc plan; the empty shapes are their own cells."""
    p = plan["path"]
    if p in (PATH_NONE, PATH_ZERO):
        return ("none" if p == PATH_NONE else "zero", 0, "direct", dtype)
    assert p in (PATH_STREAM, PATH_MFMA), plan
    return ("stream" if p == PATH_STREAM else "mfma", case[0][4], "split" if plan["splits"] > 1 else "direct", dtype)


def required_regimes(direction):
    """dx: every cell, and both empty paths.  dc: the stream path never splits m (section 12's plan), and dc of an empty shape is 0."""
    cells = set(itertools.product(("stream", "mfma"), (2, 4), ("direct", "split"), DTYPES))
    if direction == "dc":
        cells = {c for c in cells if not (c[0] == "stream" and c[2] == "split")}
        return cells | {("zero", 0, "direct", d) for d in DTYPES}
    return cells | {(e, 0, "direct", d) for e in ("none", "zero") for d in DTYPES}


def xvec_arms(case):
    """(dx arm, dc arm) the MFMA launch takes on 256-byte aligned allocations: dx needs g 16-byte aligned and ncols a multiple of 8,
    dc x and g 4-byte aligned and kdim, ncols even; a buf[1:] view is 2 bytes off either."""
    (_, m, kdim, ncols, *_), view = case
    return (not view and ncols % 8 == 0, not view and kdim % 2 == 0 and ncols % 2 == 0)
