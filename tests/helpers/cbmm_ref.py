"""References and the case list for the codebook matmul tests (ops.codebook_matmul, csrc/nnc_cbmm.hip, compressed.py).

- ``conv_nhwc``: a float64 NumPy convolution (NHWC, Keras kernel layout), never MIOpen, which may pick an inexact algorithm.
- ``matmul64``: x @ W + bias in float64 without BLAS, so Inf * 0 gives NaN wherever it occurs; ``relu_like_torch``.
- ``exact_grid_bits`` / ``assert_exact``: the precondition under which every float32 partial sum is exact.
- ``REGIME_CASES`` / ``regime_of`` / ``required_regimes``: calls that, between them, hit every kernel regime the plan can
  choose (include/nnc.h, nnc_cbmm_plan); the CPU suite checks the coverage at several CU counts, the GPU suite at the
  device's own and runs every case.
Test infrastructure only."""
from __future__ import annotations

import itertools

import numpy as np


# ------------------------------------------------------------------ float64 references
def conv_nhwc(x, kernel, pad):
    """Reference convolution: x (N, H, W, C), kernel (h, w, in, out) as Keras stores it, stride 1, zero padding; float64."""
    n, hh, ww, c = x.shape
    h, w, _, cout = kernel.shape
    xp = np.pad(np.asarray(x, dtype=np.float64), ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    ho, wo = hh + 2 * pad - h + 1, ww + 2 * pad - w + 1
    out = np.zeros((n, ho, wo, cout), dtype=np.float64)
    for dy in range(h):
        for dx in range(w):
            out += np.einsum("nijc,co->nijo", xp[:, dy: dy + ho, dx: dx + wo, :], np.asarray(kernel[dy, dx], dtype=np.float64))
    return out


def matmul64(x, w, bias=None):
    """x (m, kdim) @ w (kdim, ncols) + bias in float64, one row of w at a time (no BLAS, which may skip zero operands and so
    lose the NaN of Inf * 0)."""
    x64, w64 = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    acc = np.zeros((x64.shape[0], w64.shape[1]), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(x64.shape[1]):
            acc += x64[:, i: i + 1] * w64[i]
        if bias is not None:
            acc += np.asarray(bias, dtype=np.float64)
    return acc


def relu_like_torch(v):
    """torch.relu: negative values (-Inf included) become 0, NaN stays NaN."""
    with np.errstate(invalid="ignore"):
        return np.where(v < 0, 0.0, v)


def exact_grid_bits(*arrays) -> int:
    """The smallest g with every finite value of every array a multiple of 2^-g (at most 60)."""
    g = 0
    for a in arrays:
        a = np.asarray(a, dtype=np.float64)
        a = a[np.isfinite(a)]
        while g < 60 and np.any(np.ldexp(a, g) != np.round(np.ldexp(a, g))):
            g += 1
    return g


def assert_exact(x, w, bias=None):
    """Every product and partial sum of x @ w + bias is exact in float32 whatever the order: all of them are multiples of
    2^-g (g from the operands' grids) and at most |x| @ |w| + |bias| in magnitude, which stays below 2^24 grid steps."""
    x64, w64 = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    mag = np.abs(x64) @ np.abs(w64)
    if bias is not None:
        mag = mag + np.abs(np.asarray(bias, dtype=np.float64))
    g = max(exact_grid_bits(x64) + exact_grid_bits(w64), exact_grid_bits(bias) if bias is not None else 0)
    top = float(mag.max()) if mag.size else 0.0
    assert top * 2.0 ** g < 2.0 ** 24, (top, g)


# ------------------------------------------------------------------ the regime matrix
MTS = (1, 2, 4, 8, 16)
U16_TABLE_KS = {257: 32, 263: 32, 264: 16, 527: 16, 528: 8, 1040: 8}   # K -> copies of the uint16 table (CB_U16_WORDS = 8448)
U16_SMALL_KS = (1, 17, 256)                                            # 2-byte labels with a K that 1 byte would hold
SPLIT_LIMIT_CUS = 256                                                  # the plan never splits more than for this many CUs


def regime_of(case, plan):
    """The cells of the matrix a call falls in (a set of tuples)."""
    lb, k = case["lb"], case["k"]
    mode = "split" if plan["splits"] > 1 else "direct"
    if plan["path"] == 1:
        cells = {("stream", lb, plan["mt"], "aligned" if plan["aligned"] else "unaligned", mode)}
        if lb == 2 and k in U16_TABLE_KS:
            cells.add(("u16 table", k, plan["copies"]))
        if lb == 2 and k in U16_SMALL_KS:
            cells.add(("u16 small k", k))
        return cells
    assert plan["path"] == 2, plan
    return {("tiled", lb, mode)}


def required_regimes():
    req = {("stream", lb, mt, al, mode) for lb, mt, al, mode in itertools.product((1, 2), MTS, ("aligned", "unaligned"), ("direct", "split"))}
    req |= {("tiled", lb, mode) for lb, mode in itertools.product((1, 2), ("direct", "split"))}
    req |= {("u16 table", k, c) for k, c in U16_TABLE_KS.items()}
    req |= {("u16 small k", k) for k in U16_SMALL_KS}
    return req


def _regime_cases():
    """Every m in 1..16 with both label widths, each direct (kdim < 32: every wave keeps no full batch, some waves no row at all)
    and split (kdim > 16 m / lb, not a multiple of 32), each with rows aligned (offset 0, ncols * lb a multiple of 16) and not
    (a storage offset 1..VB-1 bytes, or an ncols that leaves a lane's window running past the row end); then m = 17..130
    through the tiled kernel.  x and the bias alternate between plain tensors and misaligned views (buf[1:])."""
    cases = []
    u8_ks = (1, 2, 17, 200, 256)
    u16_ks = tuple(U16_TABLE_KS) + U16_SMALL_KS
    direct_kdims = (1, 2, 3, 31, 17, 5, 20)
    split_kdims = (600, 777, 1000)
    aligned_ncols = (64, 48, 16, 1040, 96, 32)
    unaligned_ncols = (50, 77, 1, 7, 303, 130, 64, 1027)
    i = 0
    for lb in (1, 2):
        for m in range(1, 17):
            for mode in ("direct", "split"):
                for aligned in (True, False):
                    ks = u8_ks if lb == 1 else u16_ks
                    k = ks[i % len(ks)]
                    kdim = direct_kdims[i % len(direct_kdims)] if mode == "direct" else split_kdims[i % len(split_kdims)]
                    if aligned:
                        ncols, off = aligned_ncols[i % len(aligned_ncols)], 0
                    else:
                        ncols = unaligned_ncols[i % len(unaligned_ncols)]
                        # rows of 16-byte multiples need an odd element offset (never a multiple of VB = 4, 8 or 16 bytes)
                        vb_elems = 16 // lb
                        off = 1 + 2 * (i % (vb_elems // 2)) if ncols * lb % 16 == 0 else i % vb_elems
                    cases.append(dict(m=m, kdim=kdim, ncols=ncols, lb=lb, k=k, off=off, x_view=i % 2 == 1, bias=i % 3 != 2,
                                      bias_view=i % 4 == 1, want=(mode, aligned)))
                    i += 1
    # every storage offset 0..VB-1 of one uint8 row width, and every even byte offset of a uint16 one, at m = 1 (VB = 16)
    for off in range(16):
        cases.append(dict(m=1, kdim=97, ncols=45, lb=1, k=256, off=off, x_view=off % 2 == 0, bias=True, bias_view=False, want=None))
    for off in range(8):
        cases.append(dict(m=2, kdim=70, ncols=21, lb=2, k=300, off=off, x_view=False, bias=True, bias_view=off % 2 == 1, want=None))
    # the tiled kernel: kdim < 256 is direct; kdim >= 256 over a few tiles splits
    for lb, k in ((1, 17), (1, 256), (2, 1040), (2, 17)):
        cases.append(dict(m=17, kdim=3, ncols=50, lb=lb, k=k, off=1, x_view=True, bias=True, bias_view=True, want=None))
        cases.append(dict(m=40, kdim=100, ncols=129, lb=lb, k=k, off=0, x_view=False, bias=False, bias_view=False, want=None))
        cases.append(dict(m=17, kdim=300, ncols=50, lb=lb, k=k, off=3 if lb == 1 else 1, x_view=False, bias=True, bias_view=False, want=None))
        cases.append(dict(m=130, kdim=1001, ncols=200, lb=lb, k=k, off=0, x_view=True, bias=True, bias_view=True, want=None))
    return cases


REGIME_CASES = _regime_cases()


def case_id(c):
    return f"m{c['m']}-kd{c['kdim']}-n{c['ncols']}-lb{c['lb']}-k{c['k']}-o{c['off']}"
