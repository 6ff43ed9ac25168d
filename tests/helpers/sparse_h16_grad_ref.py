"""The case list of the half-precision bitmap-sparse codebook backward tests (nnc_cbsp_dx_h16 / nnc_cbsp_dc_h16,
csrc/nnc_cbspgrad_h16.hip), shared by tests/test_sparse_codebook_grad_h16_abi.py (CPU: the plans) and
tests/test_gpu_sparse_codebook_backward_h16.py.

``CASES``: every m of ``MS`` with every kdim of ``KDIMS``; the column counts, label widths, codebook sizes, densities, the kind of
skipped symbol (chosen by the packer, given, or >= K), stored symbols beyond K and the buf[1:] views of x and g cycle through them
with strides chosen so that no two of them move together; then the few shapes the cycle does not reach: a dx split on the MFMA
path for both label widths (ncols >= 128 with few tiles), nnz = 0 through both kernels, K = 1, and the 16-byte aligned / even
shapes that take the XVEC arms of the two MFMA kernels.  The smallest shapes at which the kernels can go wrong: ncols = 1 is one bit
of a word, 31 and 63 a partial word below a step / a word, 64 one whole word, 65 a second word of one bit, 129 a second tile of one
column, 200 and 330 words cut by a split of ncols (a multiple of 32, so a word can straddle two splits); kdim below, at and above a
tile of 128 index rows; m on both sides of 16, of a k step of 32 and of a tile of 128 (m = 130, 200: a split of m in dc).
``regime_of`` / ``required_regimes``: the cells {stream, MFMA} x {uint8, uint16} x {direct, split} x {bf16, fp16} of dx and of dc the
list has to hit (every case runs with both dtypes; the dc stream plan never splits m).
Test infrastructure only."""
from __future__ import annotations

import itertools

import numpy as np

from tests.helpers.h16_ref import DTYPES, PATH_MFMA, PATH_STREAM

MS = (1, 7, 16, 17, 33, 130, 200)
KDIMS = (1, 3, 17, 127, 129, 300)
NCOLS = (1, 31, 63, 64, 65, 129, 200, 330)
DENSITIES = (0.02, 0.32, 1.0)
U8_KS, U16_KS = (2, 256), (257, 300)
Z_KINDS = ("chosen", "given", "beyond")


def _cases():
    cases = []
    for i, (m, kdim) in enumerate(itertools.product(MS, KDIMS)):
        lb = 1 + (i + i // 2) % 2
        cases.append(dict(m=m, kdim=kdim, ncols=NCOLS[(i + i // 6) % len(NCOLS)], lb=lb, k=(U8_KS if lb == 1 else U16_KS)[(i // 3) % 2],
                          density=DENSITIES[(i + i // 7) % 3], z=Z_KINDS[(i + i // 4) % 3], beyond=i % 5 == 3, view=i % 2 == 1))
    extra = [
        dict(m=40, kdim=100, ncols=330, lb=1, k=256, density=0.32, z="given", beyond=False, view=False),    # MFMA, dx split, uint8
        dict(m=33, kdim=17, ncols=200, lb=2, k=257, density=0.32, z="chosen", beyond=True, view=True),      # MFMA, dx split, uint16
        dict(m=7, kdim=100, ncols=129, lb=1, k=17, density=0.0, z="given", beyond=False, view=False),       # nnz = 0, stream
        dict(m=33, kdim=100, ncols=129, lb=2, k=257, density=0.0, z="beyond", beyond=False, view=True),     # nnz = 0, MFMA, z >= K
        dict(m=130, kdim=33, ncols=65, lb=1, k=1, density=0.32, z="beyond", beyond=False, view=False),      # K = 1: the stored symbols are 0
        dict(m=64, kdim=128, ncols=136, lb=1, k=17, density=0.32, z="given", beyond=False, view=False),     # both XVEC arms
        dict(m=16, kdim=300, ncols=1000, lb=2, k=300, density=0.02, z="chosen", beyond=False, view=False),  # stream, dx split, uint16
    ]
    return cases + extra


CASES = _cases()


def case_id(c):
    return f"m{c['m']}-kd{c['kdim']}-n{c['ncols']}-lb{c['lb']}-k{c['k']}-d{c['density']}-z{c['z']}{'-b' if c['beyond'] else ''}{'-v' if c['view'] else ''}"


def case_labels(c, seed=0):
    """(labels (kdim, ncols) int64, zero_symbol or None for the packer's choice): ``density`` of the positions hold a symbol other than
    the skipped one; ``beyond``: some stored symbols lie past K (they read 0 in dx and fall into no bin in dc)."""
    rng = np.random.RandomState(1000 + seed + c["m"] * 7 + c["kdim"] * 13 + c["ncols"])
    kdim, ncols, k, lb = c["kdim"], c["ncols"], c["k"], c["lb"]
    top = 256 if lb == 1 else 65536
    if c["z"] == "beyond" and k < top:
        z = int(rng.randint(k, min(top, k + 40)))
    else:
        z = int(rng.randint(0, k))
    others = np.array([s for s in range(k) if s != z] or [z], dtype=np.int64)
    lab = np.full((kdim, ncols), z, dtype=np.int64)
    stored = rng.rand(kdim, ncols) < c["density"]
    if others[0] != z:
        lab[stored] = others[rng.randint(0, len(others), size=int(stored.sum()))]
    if c["beyond"] and k < top - 1:
        far = stored & (rng.rand(kdim, ncols) < 0.1)
        pool = np.array([s for s in range(k, min(top, k + 40)) if s != z], dtype=np.int64)
        lab[far] = pool[rng.randint(0, len(pool), size=int(far.sum()))]
    # the packer's own choice is the most frequent symbol: leave it None only where that is unambiguous bookkeeping for the test
    return lab, (None if c["z"] == "chosen" else z)


def regime_of(case, plan, dtype):
    assert plan["path"] in (PATH_STREAM, PATH_MFMA), plan
    return ("stream" if plan["path"] == PATH_STREAM else "mfma", case["lb"], "split" if plan["splits"] > 1 else "direct", dtype)


def required_regimes(direction):
    cells = set(itertools.product(("stream", "mfma"), (1, 2), ("direct", "split"), DTYPES))
    if direction == "dc":   # section 12's stream plan never splits m
        cells = {c for c in cells if not (c[0] == "stream" and c[2] == "split")}
    return cells


def xvec_arms(c):
    """(dx arm, dc arm) of the MFMA kernels on 256-byte aligned allocations: dx needs g 16-byte aligned and ncols a multiple of 8, dc
    x and g 4-byte aligned and kdim, ncols even; a buf[1:] view is 2 bytes off either."""
    return (not c["view"] and c["ncols"] % 8 == 0, not c["view"] and c["kdim"] % 2 == 0 and c["ncols"] % 2 == 0)
