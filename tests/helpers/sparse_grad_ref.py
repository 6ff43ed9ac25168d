"""References and the case list for the bitmap-sparse codebook backward tests (ops.sparse_codebook_matmul_dx /
sparse_codebook_centroid_grad / sparse_codebook_linear, csrc/nnc_cbspgrad.hip).

- ``labels_for``: labels at a density of stored (non-z) indices, optionally with stored indices >= K.
- ``dx64``: the float64 formula of include/nnc.h (c_z * row sums of g + the stored weights' g * d, the rank-1 term dropped for
  c_z == 0).
- ``dx_bound``: the DESIGN.md section 13 bound of |dx - g @ W^T| (W decoded, float64).
- ``REGIME_CASES`` / ``dx_regime`` / ``dc_regime``: calls that, between them, hit every regime of the two plans.
- ``case_data`` and ``dx64`` also serve tests/helpers/stream_cells_ref.py, whose cases reach every stream instantiation.
Test infrastructure only."""
from __future__ import annotations

import numpy as np

from tests.helpers.sparse_ref import d_table

U = 2.0 ** -24
PATH_NONE, PATH_STREAM, PATH_TILED, PATH_ZERO = 0, 1, 2, 4


def labels_for(rng, kdim, ncols, k, lb, density, z, oob=False):
    """(kdim, ncols) labels: z where skipped, else a random index != z below K (or, with ``oob``, up to K + 2; uint8: < 256)."""
    top = min(k + 3 if oob else k, 256 if lb == 1 else 65536)
    choices = np.array([v for v in range(top) if v != z], dtype=np.int64)
    lab = np.full((kdim, ncols), z, dtype=np.int64)
    if choices.size:
        keep = rng.random_sample((kdim, ncols)) < density
        lab[keep] = choices[rng.randint(0, choices.size, size=int(keep.sum()))]
    return lab


def stored_d(lab, centers, z):
    """D[i, o] = d[labels[i, o]] (float32 values) where stored, 0 where skipped; and c_z."""
    lab = np.asarray(lab)
    d, cz = d_table(centers, max(int(lab.max(initial=0)) + 1, np.asarray(centers).size), z)
    return np.where(lab != z, d[lab].astype(np.float64), 0.0), float(cz)


def dx64(g, lab, centers, z):
    D, cz = stored_d(lab, centers, z)
    g64 = np.asarray(g, dtype=np.float64)
    out = g64 @ D.T
    if cz != 0:
        out = cz * g64.sum(axis=1, keepdims=True) + out
    return out


def decoded(lab, centers):
    c = np.asarray(centers, dtype=np.float64)
    lab = np.asarray(lab)
    return np.where(lab < c.size, c[np.minimum(lab, c.size - 1)], 0.0)


def dx_bound(g, lab, centers, z):
    """(g @ W^T in float64, 2 (ncols + 4) u (|g| |D|^T + |c_z| sum|g|) + u (|g| |C - c_z|^T))."""
    lab = np.asarray(lab)
    ncols = lab.shape[1]
    D, cz = stored_d(lab, centers, z)
    W = decoded(lab, centers)
    g64 = np.asarray(g, dtype=np.float64)
    ga = np.abs(g64)
    exact = np.where(lab != z, np.abs(W - cz), 0.0)
    b = 2.0 * (ncols + 4) * U * (ga @ np.abs(D).T + abs(cz) * ga.sum(axis=1, keepdims=True)) + U * (ga @ exact.T) + 1e-30
    return g64 @ W.T, b


# ------------------------------------------------------------------ the regime matrix
# name, m, kdim, ncols, label bytes, K, density, z ("auto" or an index; >= K allowed), stored indices >= K, c_z == 0
REGIME_CASES = [
    ("stream_m1_u8_nosplit", 1, 37, 200, 1, 256, 0.1, "auto", False, False),
    ("stream_m1_u8_split_oob", 1, 300, 2500, 1, 200, 0.1, 5, True, True),
    ("stream_m3_k1_oob", 3, 65, 130, 1, 1, 0.5, 0, True, False),
    ("stream_m5_u16_k257_split", 5, 129, 700, 2, 257, 0.01, "auto", True, False),
    ("stream_m8_u16_k1040_dense", 8, 70, 333, 2, 1040, 1.0, 7, False, False),
    ("stream_m16_k2_nosplit_zbig", 16, 96, 100, 1, 2, 0.5, 5, False, False),
    ("stream_m16_u16_k1040_split", 16, 40, 1000, 2, 1040, 0.1, "auto", False, True),
    ("stream_m2_kdim1_n65", 2, 1, 65, 1, 17, 0.5, 3, False, False),
    ("stream_m12_u16_n63_empty", 12, 200, 63, 2, 256, 0.0, 9, False, False),
    ("stream_m4_n1", 4, 50, 1, 1, 2, 0.5, 1, False, False),
    ("stream_m7_n64", 7, 90, 64, 1, 256, 0.1, "auto", False, True),
    ("tiled_m17_u8_nosplit", 17, 100, 100, 1, 256, 0.1, "auto", False, False),
    ("tiled_m40_u16_split_oob", 40, 100, 300, 2, 1040, 0.1, 11, True, True),
    ("tiled_m200_kdim1_split", 200, 1, 513, 1, 2, 0.5, 0, False, False),
    ("tiled_m256_u16_msplit_zbig", 256, 100, 70, 2, 257, 0.01, 300, True, False),
    ("tiled_m300_k1_msplit", 300, 33, 129, 1, 1, 1.0, 0, True, False),
    ("empty_m", 0, 50, 60, 1, 8, 0.1, "auto", False, False),
    ("empty_kdim", 4, 0, 60, 1, 8, 0.1, 0, False, False),
    ("empty_ncols", 4, 50, 0, 2, 300, 0.1, 0, False, False),
    ("empty_ncols_tiled", 20, 50, 0, 1, 8, 0.1, 0, False, False),
]


def regime(plan):
    p = plan["path"]
    return (p, plan["splits"] > 1) if p in (PATH_STREAM, PATH_TILED) else (p, False)


DX_REQUIRED = {(PATH_STREAM, False), (PATH_STREAM, True), (PATH_TILED, False), (PATH_TILED, True), (PATH_NONE, False), (PATH_ZERO, False)}
DC_REQUIRED = {(PATH_STREAM, False), (PATH_TILED, False), (PATH_TILED, True), (PATH_ZERO, False)}


def case_data(case, seed):
    """Exact data: integer x, g in [-3, 3], dyadic centres (multiples of 1/4 in [-2, 2]; c_z = 0 or 3/4 as the case says), labels
    at the case's density; z is the skipped symbol to pass (None: the default choice)."""
    _, m, kdim, ncols, lb, k, density, z, oob, cz_zero = case
    rng = np.random.RandomState(seed)
    x = rng.randint(-3, 4, size=(m, kdim)).astype(np.float32)
    g = rng.randint(-3, 4, size=(m, ncols)).astype(np.float32)
    c = (rng.randint(-8, 9, size=k) / 4.0).astype(np.float32)
    zz = 0 if z == "auto" else z
    if zz < k:
        c[zz] = 0.0 if cz_zero else 0.75
    lab = labels_for(rng, kdim, ncols, k, lb, density, zz, oob)
    return x, g, c, lab, (None if z == "auto" else z)
