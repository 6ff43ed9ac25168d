"""The case list of the half-precision bitmap-sparse codebook matmul tests (nnc_cbsp_h16, csrc/nnc_cbsp_h16.hip, DESIGN.md section
23), shared by tests/test_sparse_codebook_h16_abi.py (CPU: the plan) and tests/test_gpu_sparse_codebook_h16.py.

``CASES``: every m of ``MS`` with every kdim of ``KDIMS``; the column counts, label widths, codebook sizes, densities, c_z, the
buf[1:] view of x, the bias and the fused ReLU cycle through them with strides chosen so that no two of them move together, plus
two layers with no stored symbol at all.  ``regime_of`` / ``required_regimes``: the cells {stream, MFMA} x {uint8, uint16} x
{direct, split} x {bf16, fp16} the list has to hit (every case runs with both dtypes).  The smallest shapes at which the kernels can
go wrong: ncols = 1 is one lane of a segment, 50 a partial segment, 64 one full wave of a tile whose second wave has no column,
129 a tile whose second wave has one column and a second tile of one, 200 a second tile holding two partial segments... kdim below,
at and above a k step of 32, 300 and 1001 cut into splits by the MFMA plan, 1001 by the stream plan too.
Test infrastructure only."""
from __future__ import annotations

import itertools

from tests.helpers.h16_ref import DTYPES, PATH_MFMA, PATH_STREAM

MS = (1, 7, 16, 17, 33, 130)
KDIMS = (1, 3, 17, 33, 100, 300, 1001)
NCOLS = (1, 50, 64, 129, 200)
DENSITIES = (0.02, 0.32, 1.0)
U8_KS, U16_KS = (17, 256), (257, 1040)


def _cases():
    cases = []
    for i, (m, kdim) in enumerate(itertools.product(MS, KDIMS)):
        lb = 1 + (i + i // 2) % 2
        cases.append(dict(m=m, kdim=kdim, ncols=NCOLS[i % len(NCOLS)], lb=lb, k=(U8_KS if lb == 1 else U16_KS)[(i // 3) % 2],
                          density=DENSITIES[(i + i // 7) % 3], cz_zero=(i // 2) % 2 == 0, x_view=i % 2 == 1, bias=i % 4 != 2, relu=i % 3 == 1))
    # a layer of which nothing is stored (nnz = 0: the symbols are an empty range), through both kernels
    cases.append(dict(m=7, kdim=100, ncols=129, lb=1, k=17, density=0.0, cz_zero=False, x_view=False, bias=True, relu=False))
    cases.append(dict(m=33, kdim=100, ncols=129, lb=2, k=257, density=0.0, cz_zero=True, x_view=True, bias=True, relu=True))
    return cases


CASES = _cases()


def case_id(c):
    return f"m{c['m']}-kd{c['kdim']}-n{c['ncols']}-lb{c['lb']}-k{c['k']}-d{c['density']}-{'z0' if c['cz_zero'] else 'z1'}"


def regime_of(case, plan, dtype):
    assert plan["path"] in (PATH_STREAM, PATH_MFMA), plan
    return ("stream" if plan["path"] == PATH_STREAM else "mfma", case["lb"], "split" if plan["splits"] > 1 else "direct", dtype)


def required_regimes():
    return set(itertools.product(("stream", "mfma"), (1, 2), ("direct", "split"), DTYPES))
