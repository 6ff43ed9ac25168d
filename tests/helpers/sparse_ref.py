"""References and the case list for the bitmap-sparse codebook matmul tests (ops.pack_sparse_codes / sparse_codebook_matmul,
csrc/nnc_cbsp.hip, compressed.Sparse*).

- ``pack_np`` / ``split_packed``: a NumPy packer of the form include/nnc.h describes, and the device buffer cut into its parts.
- ``sparse_formula64``: y = c_z * sum_i x + sum over stored (i, o) of x * d[label] (+ bias, ReLU) in float64, d rounded to float32
  as the form defines it; a skipped weight is absent when c_z == 0 (no Inf * 0).
- ``float_bound``: the float32 error bound of DESIGN.md section 11 against the float64 product with the decoded W.
- ``REGIME_CASES`` / ``regime_of`` / ``required_regimes``: calls that hit every regime nnc_cbsp_plan can choose.
Test infrastructure only."""
from __future__ import annotations

import itertools

import numpy as np

U = 2.0 ** -24


# ------------------------------------------------------------------ the form
def layout(kdim, ncols, lb, nnz):
    segs = -(-ncols // 64)
    g = kdim * segs
    off_lo, off_hi = 8 * g, 12 * g
    off_sym = (off_hi + 4 * kdim + 255) // 256 * 256
    return dict(segs=segs, g=g, off_lo=off_lo, off_hi=off_hi, off_sym=off_sym, bytes=off_sym + nnz * lb)


def pack_np(lab, kdim, ncols, z):
    """-> dict(bitmap uint64[kdim, S], counts int64[kdim, S] (exclusive, row-major), symbols, nnz)."""
    lab = np.asarray(lab).reshape(kdim, ncols)
    segs = -(-ncols // 64)
    keep = np.zeros((kdim, segs * 64), dtype=bool)
    keep[:, :ncols] = lab != z
    k3 = keep.reshape(kdim, segs, 64).astype(np.uint64)
    bitmap = (k3 << np.arange(64, dtype=np.uint64)).sum(axis=2, dtype=np.uint64) if segs else np.zeros((kdim, 0), np.uint64)
    per = keep.reshape(kdim, segs, 64).sum(axis=2).astype(np.int64).ravel()
    counts = (np.cumsum(per) - per).reshape(kdim, segs)
    return dict(bitmap=bitmap, counts=counts, symbols=lab[lab != z], nnz=int((lab != z).sum()))


def split_packed(raw: np.ndarray, kdim, ncols, lb, nnz):
    """The packed bytes -> (bitmap uint64[kdim, S], counts int64[kdim, S] decoded from lo / hi, symbols)."""
    L = layout(kdim, ncols, lb, nnz)
    segs, g = L["segs"], L["g"]
    bitmap = raw[: 8 * g].view(np.uint64).reshape(kdim, segs)
    lo = raw[L["off_lo"]: L["off_lo"] + 4 * g].view(np.uint32).reshape(kdim, segs).astype(np.int64)
    hi = raw[L["off_hi"]: L["off_hi"] + 4 * kdim].view(np.uint32).astype(np.int64)
    counts = (hi[:, None] << 32) + lo
    if segs:
        counts = counts + np.where(lo < lo[:, :1], 1 << 32, 0)
    sym = raw[L["off_sym"]: L["off_sym"] + nnz * lb].view(np.uint8 if lb == 1 else np.uint16)
    return bitmap, counts, sym


# ------------------------------------------------------------------ the arithmetic
def d_table(centers, k_all, z):
    """d[s] for s < k_all: float32(c[s] - c_z), -c_z past K; and c_z."""
    c = np.asarray(centers, dtype=np.float32).ravel()
    k = c.size
    cz = np.float32(c[z]) if z < k else np.float32(0.0)
    d = np.full(k_all, np.float32(0.0) - cz, dtype=np.float32)
    d[:k] = c - cz
    return d, cz


def sparse_formula64(x, lab, centers, z, bias=None, relu=False):
    """The defining formula in float64, row by row of W (no BLAS: NaN and Inf as they arise)."""
    x64 = np.asarray(x, dtype=np.float64)
    lab = np.asarray(lab)
    kdim, ncols = lab.shape
    d, cz = d_table(centers, max(int(lab.max(initial=0)) + 1, np.asarray(centers).size), z)
    acc = np.zeros((x64.shape[0], ncols), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(kdim):
            keep = lab[i] != z
            if keep.any():
                acc[:, keep] += x64[:, i: i + 1] * d[lab[i, keep]].astype(np.float64)
        if cz != 0:
            acc = float(cz) * x64.sum(axis=1, keepdims=True) + acc
        if bias is not None:
            acc = acc + np.asarray(bias, dtype=np.float64)
        if relu:
            acc = np.where(acc < 0, 0.0, acc)
    return acc


def float_bound(x, lab, centers, z, bias=None):
    """The float64 product with the decoded W and the DESIGN.md section 11 bound of |y - it|:
    2 (kdim + 4) u (|x| @ |D| + |c_z| sum|x| + |b|) + u (|x| @ |C - c_z|), D the float32 d of the stored weights (0 elsewhere)."""
    x64 = np.abs(np.asarray(x, dtype=np.float64))
    lab = np.asarray(lab)
    kdim = lab.shape[0]
    c = np.asarray(centers, dtype=np.float32).ravel()
    d, cz = d_table(c, max(int(lab.max(initial=0)) + 1, c.size), z)
    keep = lab != z
    w = np.where(lab < c.size, c[np.minimum(lab, c.size - 1)], 0.0).astype(np.float64)
    ref = np.asarray(x, dtype=np.float64) @ w
    dmag = np.where(keep, np.abs(d[lab].astype(np.float64)), 0.0)
    exact_d = np.where(keep, np.abs(w - float(cz)), 0.0)
    mag = x64 @ dmag + abs(float(cz)) * x64.sum(axis=1, keepdims=True)
    if bias is not None:
        ref = ref + np.asarray(bias, dtype=np.float64)
        mag = mag + np.abs(np.asarray(bias, dtype=np.float64))
    return ref, 2.0 * (kdim + 4) * U * mag + U * (x64 @ exact_d) + 1e-30


# ------------------------------------------------------------------ the regime matrix
MTS = (1, 2, 4, 8, 16)
U16_TABLE_KS = {257: 32, 264: 16, 528: 8, 1040: 8}


def regime_of(case, plan):
    lb, k = case["lb"], case["k"]
    mode = "split" if plan["splits"] > 1 else "direct"
    if plan["path"] == 1:
        cells = {("stream", lb, plan["mt"], mode)}
        if lb == 2 and k in U16_TABLE_KS:
            cells.add(("u16 table", k, plan["copies"]))
        return cells
    assert plan["path"] == 2, plan
    return {("tiled", lb, mode)}


def required_regimes():
    req = {("stream", lb, mt, mode) for lb, mt, mode in itertools.product((1, 2), MTS, ("direct", "split"))}
    req |= {("tiled", lb, mode) for lb, mode in itertools.product((1, 2), ("direct", "split"))}
    req |= {("u16 table", k, c) for k, c in U16_TABLE_KS.items()}
    return req


def _regime_cases():
    """m = 1..16 with both label widths, each direct (kdim < 256: no wave keeps a full batch of 64 rows) and split (kdim >= 1000,
    few segments); then m = 17, 256, 4096 through the tiled kernel, direct (kdim < 128) and split.  Densities and ncols vary;
    labels start at odd element offsets every other case."""
    cases = []
    u8_ks, u16_ks = (2, 17, 256), tuple(U16_TABLE_KS) + (17,)
    densities = (0.1, 0.32, 0.02, 0.5, 1.0)
    direct_kdims = (1, 7, 63, 200, 130)
    split_kdims = (1000, 1500, 2100)
    ncols_list = (64, 50, 130, 1, 300, 77, 192)
    i = 0
    for lb in (1, 2):
        for m in range(1, 17):
            for mode in ("direct", "split"):
                ks = u8_ks if lb == 1 else u16_ks
                kdim = direct_kdims[i % len(direct_kdims)] if mode == "direct" else split_kdims[i % len(split_kdims)]
                cases.append(dict(m=m, kdim=kdim, ncols=ncols_list[i % len(ncols_list)], lb=lb, k=ks[i % len(ks)],
                                  density=densities[i % len(densities)], off=i % 2, bias=i % 3 != 2, want=mode))
                i += 1
    for lb, k in ((1, 17), (1, 256), (2, 1040), (2, 300)):
        for m, kdim, ncols, want in ((17, 100, 50, "direct"), (256, 600, 129, "split"), (4096, 64, 200, "direct"), (4096, 300, 70, None)):
            cases.append(dict(m=m, kdim=kdim, ncols=ncols, lb=lb, k=k, density=densities[i % len(densities)], off=i % 2, bias=i % 3 != 2, want=want))
            i += 1
    return cases


REGIME_CASES = _regime_cases()


def case_id(c):
    return f"m{c['m']}-kd{c['kdim']}-n{c['ncols']}-lb{c['lb']}-k{c['k']}-d{c['density']}"


def labels_at_density(rng, kdim, ncols, k, density, z=0):
    """Labels in 0..k-1 with the share ``density`` (about) not equal to z, and z the most frequent."""
    lab = np.full(kdim * ncols, z, dtype=np.int64)
    keep = rng.random_sample(kdim * ncols) < density
    if k > 1:
        others = rng.randint(0, k - 1, size=int(keep.sum()))
        lab[keep] = others + (others >= z)
    return lab.reshape(kdim, ncols)
