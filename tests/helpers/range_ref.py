"""Scaled exact data for the range tests of the codebook family (tests/test_gpu_codebook_range.py).

The exact data of cbgrad_ref / sparse_grad_ref (integers in [-3, 3], centres in multiples of 1/4) scaled by powers of two: x (or
g) by 2^a, the other operand by 2^b.  Every product is then an integer times 2^(a + b), so the float64 formulas stay exact at any
scale and a float32 result must be float32(formula) bit for bit.
Test infrastructure only."""
from __future__ import annotations

import numpy as np

from tests.helpers import cbgrad_ref, sparse_grad_ref

FLT_MIN = 2.0 ** -126
FLT_MAX = float(np.finfo(np.float32).max)

DENSE_CASES = [c for c in cbgrad_ref.REGIME_CASES if c[1] * c[2] * c[3] > 0]
SPARSE_CASES = [c for c in sparse_grad_ref.REGIME_CASES if c[1] * c[2] * c[3] > 0]

# (id, a, b): x scaled by 2^a, g by 2^b
DC_EXPONENTS = [
    ("below_denorm_80", -80, -80),        # products below 2^-149, inputs normal
    ("below_denorm_100", -100, -100),
    ("subnormal_products", -70, -70),     # products subnormal but representable
    ("baseline", 0, 0),
    ("large", 30, 30),                    # products near 2^60
    ("subnormal_x", -140, 10),            # max |x| below FLT_MIN, products subnormal
    ("subnormal_x_tiny_g", -140, -20),    # ... and products below 2^-149
    ("subnormal_g", 20, -142),            # max |g| below FLT_MIN
]


def scale(a, e):
    """float32(a * 2^e), asserted exact (subnormal results included)."""
    out = np.ldexp(np.asarray(a, dtype=np.float64), e).astype(np.float32)
    assert np.array_equal(out.astype(np.float64), np.ldexp(np.asarray(a, dtype=np.float64), e))
    return out


def top_exponent(m, x_int, g_int, below: bool):
    """a + b with m * max|x_int| * max|g_int| * 2^(a + b) just below 2^127 (below) or in [2^127, 2^128) (not below)."""
    mag = max(float(m) * float(np.abs(x_int).max()) * float(np.abs(g_int).max()), 1.0)   # (a zero operand: any scale)
    _, p = np.frexp(mag)            # mag in [2^(p-1), 2^p)
    return 127 - int(p) + (0 if below else 1)


def f32_of(v64):
    """np.float32 of float64 values, overflow to +-inf allowed."""
    with np.errstate(over="ignore"):
        return np.asarray(v64, dtype=np.float64).astype(np.float32)


def grid_exponent(mag_int):
    """e with max(mag_int) * 2^e in [2^127, 2^128): the largest power-of-two scale at which every partial sum (at most mag_int in
    steps of 1) stays below FLT_MAX."""
    top = float(np.max(mag_int)) if np.size(mag_int) else 1.0
    _, p = np.frexp(max(top, 1.0))
    return 128 - int(p)
