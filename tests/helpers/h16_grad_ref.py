"""The case list of the half-precision codebook backward tests (nnc_cbmm_dx_h16 / nnc_cbmm_dc_h16, csrc/nnc_cbgrad_h16.hip,
DESIGN.md section 22), shared by tests/test_codebook_grad_h16_abi.py (CPU: the plans) and tests/test_gpu_codebook_backward_h16.py.

- ``CASES``: the smallest shapes that still reach every cell {stream, MFMA} x {uint8, uint16} x {direct, split} x {bf16, fp16} of
  dx and of dc (every case runs with both dtypes), both ``XVEC`` arms of each MFMA kernel, and the four empty shapes of
  ``cbgrad_ref.REGIME_CASES``.  A case is a ``cbgrad_ref`` tuple (so ``cbgrad_ref.case_data`` makes its exact data) and a flag:
  x and g as ``buf[1:]`` views.
- ``regime_of`` / ``required_regimes``: the cell a plan lies in, and the cells the list has to hit.
- the float64 formulas are ``cbgrad_ref.dx64`` / ``dc64``, the roundings ``h16_ref.round_to`` / ``half_ulp``; ``dx_bound`` / ``dc_bound``
  are the bounds of section 22 (one whole float32 ulp per addition).
Test infrastructure only."""
from __future__ import annotations

import itertools

import numpy as np

from . import cbgrad_ref
from .h16_ref import DTYPES, PATH_MFMA, PATH_STREAM

PATH_NONE, PATH_ZERO = cbgrad_ref.PATH_NONE, cbgrad_ref.PATH_ZERO

# (name, m, kdim, ncols, label bytes, K, label offset (elements), indices beyond K), x and g as buf[1:] views
CASES = [
    (("stream_m1_u8_aligned", 1, 37, 208, 1, 256, 0, False), False),
    (("stream_m5_u16_k257", 5, 129, 700, 2, 257, 1, True), False),
    (("stream_m16_u16_k1040", 16, 40, 1000, 2, 1040, 0, False), True),
    (("stream_m2_kdim1_u16", 2, 1, 77, 2, 17, 0, False), False),
    (("stream_m9_u8_split", 9, 40, 300, 1, 200, 3, True), False),
    (("mfma_m17_u8_direct", 17, 100, 100, 1, 256, 1, False), False),
    (("mfma_m40_u16_dxsplit", 40, 100, 300, 2, 1040, 0, True), False),
    (("mfma_m130_u8_msplit", 130, 33, 129, 1, 200, 0, True), False),
    (("mfma_m200_kdim1", 200, 1, 513, 1, 3, 0, False), False),
    (("mfma_m64_aligned_xvec", 64, 128, 136, 1, 17, 0, False), False),
    (("mfma_m256_u16_views", 256, 130, 70, 2, 300, 0, False), True),
    (("mfma_m300_k1", 300, 33, 129, 1, 1, 0, False), False),
] + [(c, False) for c in cbgrad_ref.REGIME_CASES if c[0].startswith("empty_")]

FULL = [c for c in CASES if not c[0][0].startswith("empty_")]


def case_id(c):
    return c[0][0]


def regime_of(case, plan, dtype):
    """(path, label bytes, direct / split, dtype) of a dx or dc plan; the empty shapes are their own cells."""
    p = plan["path"]
    if p in (PATH_NONE, PATH_ZERO):
        return ("none" if p == PATH_NONE else "zero", 0, "direct", dtype)
    assert p in (PATH_STREAM, PATH_MFMA), plan
    return ("stream" if p == PATH_STREAM else "mfma", case[0][4], "split" if plan["splits"] > 1 else "direct", dtype)


def required_regimes(direction):
    """dx: every cell, and both empty paths.  dc: the stream path never splits m (section 12's plan), and dc of an empty shape is 0."""
    cells = set(itertools.product(("stream", "mfma"), (1, 2), ("direct", "split"), DTYPES))
    if direction == "dc":
        cells = {c for c in cells if not (c[0] == "stream" and c[2] == "split")}
        return cells | {("zero", 0, "direct", d) for d in DTYPES}
    return cells | {(e, 0, "direct", d) for e in ("none", "zero") for d in DTYPES}


def xvec_arms(case):
    """(dx arm, dc arm) the launch takes on 256-byte aligned allocations: dx needs g 16-byte aligned and ncols a multiple of 8, dc
    x and g 4-byte aligned and kdim, ncols even; a buf[1:] view is 2 bytes off either."""
    (_, m, kdim, ncols, *_), view = case
    return (not view and ncols % 8 == 0, not view and kdim % 2 == 0 and ncols % 2 == 0)


U32 = 2.0 ** -23


def dx_bound(g, w_h, splits):
    """(ncols + splits + 2) 2^-23 sum_o |g| |W_h| per element of a float32 dx."""
    ncols = np.asarray(g).shape[1]
    return (ncols + splits + 2) * U32 * (np.abs(np.asarray(g, dtype=np.float64)) @ np.abs(np.asarray(w_h, dtype=np.float64)).T)


def dc_bound(x, g, labels2d, k, S, splits, f32_out=False):
    """sum over members of ((m + splits + 2) 2^-23 sum_r |x| |g| + 2^(-S-1)), + 2^-24 |dc64| for a float32 result."""
    m = np.asarray(x).shape[0]
    mag = cbgrad_ref.bin64(cbgrad_ref.dw64(np.abs(x), np.abs(g)), labels2d, k)
    lab = np.asarray(labels2d, dtype=np.int64).ravel()
    cnt = np.bincount(lab[lab < k], minlength=k).astype(np.float64)
    b = (m + splits + 2) * U32 * mag + cnt * 2.0 ** (-S - 1)
    if f32_out:
        b = b + 2.0 ** -24 * np.abs(cbgrad_ref.dc64(x, g, labels2d, k))
    return b
