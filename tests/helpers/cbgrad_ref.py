"""References and the case list for the codebook backward tests (ops.codebook_matmul_dx / codebook_centroid_grad /
codebook_linear, csrc/nnc_cbgrad.hip).

- ``dx64`` / ``dc64``: the float64 formulas of include/nnc.h (an index >= K reads 0 in dx and falls into no bin in dc).
- ``dx_bound`` / ``dc_bound``: the float32 error bounds of DESIGN.md section 12.
- ``REGIME_CASES`` / ``dx_regime`` / ``dc_regime``: calls that, between them, hit every regime the two plans can choose.
- ``case_data`` and the formulas also serve tests/helpers/stream_cells_ref.py, whose cases reach every stream instantiation.
Test infrastructure only."""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
PATH_NONE, PATH_STREAM, PATH_TILED, PATH_ZERO = 0, 1, 2, 4


def decoded(labels2d, centers):
    """W[i, o] = centers[labels[i, o]] in float64, 0 for an index >= K."""
    lab = np.asarray(labels2d, dtype=np.int64)
    c = np.asarray(centers, dtype=np.float64)
    ok = lab < c.size
    return np.where(ok, c[np.minimum(lab, c.size - 1)], 0.0)


def dx64(g, labels2d, centers):
    return np.asarray(g, dtype=np.float64) @ decoded(labels2d, centers).T


def dw64(x, g):
    return np.asarray(x, dtype=np.float64).T @ np.asarray(g, dtype=np.float64)


def bin64(dw, labels2d, k):
    lab = np.asarray(labels2d, dtype=np.int64).ravel()
    ok = lab < k
    return np.bincount(lab[ok], weights=np.asarray(dw, dtype=np.float64).ravel()[ok], minlength=k)


def dc64(x, g, labels2d, k):
    return bin64(dw64(x, g), labels2d, k)


def dx_bound(g, labels2d, centers):
    """2 (ncols + 4) u sum_o |g| |c|: the float32 error bound of one dx element."""
    ncols = np.asarray(labels2d).shape[1]
    return 2.0 * (ncols + 4) * U * (np.abs(np.asarray(g, dtype=np.float64)) @ np.abs(decoded(labels2d, centers)).T)


def dc_bound(x, g, labels2d, k, S, f32_out=False):
    """sum over members of (2 (m + 4) u sum_r |x| |g| + 2^(-S-1)), + u |dc64| for a float32 result."""
    m = np.asarray(x).shape[0]
    mag = bin64(dw64(np.abs(x), np.abs(g)), labels2d, k)
    lab = np.asarray(labels2d, dtype=np.int64).ravel()
    cnt = np.bincount(lab[lab < k], minlength=k).astype(np.float64)
    b = 2.0 * (m + 4) * U * mag + cnt * 2.0 ** (-S - 1)
    if f32_out:
        b = b + U * np.abs(dc64(x, g, labels2d, k))
    return b


# ------------------------------------------------------------------ the regime matrix
# name, m, kdim, ncols, label bytes, K, label offset (elements), indices beyond K
REGIME_CASES = [
    ("stream_m1_u8_nosplit_aligned", 1, 37, 208, 1, 256, 0, False),
    ("stream_m1_u8_split_unaligned", 1, 300, 2500, 1, 200, 3, True),
    ("stream_m3_u8_k1", 3, 65, 130, 1, 1, 0, False),
    ("stream_m5_u16_k257", 5, 129, 700, 2, 257, 1, True),
    ("stream_m8_u16_k1040", 8, 70, 333, 2, 1040, 0, True),
    ("stream_m16_u8_aligned", 16, 96, 512, 1, 256, 0, False),
    ("stream_m16_u16_k1040_split", 16, 40, 1000, 2, 1040, 5, False),
    ("stream_m2_kdim1", 2, 1, 77, 1, 17, 0, False),
    ("stream_m12_u16_k256", 12, 200, 63, 2, 256, 0, False),
    ("tiled_m17_u8", 17, 100, 100, 1, 256, 1, False),
    ("tiled_m40_u16_split", 40, 100, 300, 2, 1040, 0, True),
    ("tiled_m200_u8_kdim1", 200, 1, 513, 1, 3, 0, False),
    ("tiled_m256_u16_msplit", 256, 100, 70, 2, 257, 3, True),
    ("tiled_m300_u8_msplit_k1", 300, 33, 129, 1, 1, 0, False),
    ("empty_m", 0, 50, 60, 1, 8, 0, False),
    ("empty_kdim", 4, 0, 60, 1, 8, 0, False),
    ("empty_ncols", 4, 50, 0, 2, 300, 0, False),
    ("empty_ncols_tiled", 20, 50, 0, 1, 8, 0, False),
]


def dx_regime(plan):
    p = plan["path"]
    if p in (PATH_STREAM, PATH_TILED):
        return (p, plan["splits"] > 1, plan["aligned"] if p == PATH_STREAM else 0)
    return (p, False, 0)


def dc_regime(plan):
    p = plan["path"]
    if p in (PATH_STREAM, PATH_TILED):
        return (p, plan["splits"] > 1, plan["aligned"] if p == PATH_STREAM else 0)
    return (p, False, 0)


DX_REQUIRED = {(PATH_STREAM, False, 0), (PATH_STREAM, True, 0), (PATH_STREAM, False, 1), (PATH_STREAM, True, 1),
               (PATH_TILED, False, 0), (PATH_TILED, True, 0), (PATH_NONE, False, 0), (PATH_ZERO, False, 0)}
DC_REQUIRED = {(PATH_STREAM, False, 0), (PATH_STREAM, False, 1), (PATH_TILED, False, 0), (PATH_TILED, True, 0), (PATH_ZERO, False, 0)}


def case_data(case, seed):
    """Exact data: integer x, g in [-3, 3], dyadic centres (multiples of 1/4 in [-2, 2]), indices in [0, K) or, with ``oob``, up
    to K + 2 (uint8: up to 255)."""
    _, m, kdim, ncols, lb, k, _, oob = case
    rng = np.random.RandomState(seed)
    x = rng.randint(-3, 4, size=(m, kdim)).astype(np.float32)
    g = rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
    c = (rng.randint(-8, 9, size=k) / 4.0).astype(np.float32)
    top = min(k + 3 if oob else k, 256 if lb == 1 else 65536)
    lab = rng.randint(0, top, size=(kdim, ncols))
    return x, g, c, lab
