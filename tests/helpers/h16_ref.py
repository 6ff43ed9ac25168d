"""The case list and the references of the half-precision codebook matmul tests (nnc_cbmm_h16, csrc/nnc_cbmm_h16.hip,
DESIGN.md section 16), shared by tests/test_codebook_h16_abi.py (CPU: the plan) and tests/test_gpu_codebook_h16.py.

- ``CASES``: every m of ``MS`` with every kdim of ``KDIMS``, the column counts, label widths, label offsets and the buf[1:] views of
  x and the bias cycling through them; ``regime_of`` / ``required_regimes``: the cells {stream, MFMA} x {uint8, uint16} x
  {direct, split} x {bf16, fp16} the list has to hit (every case runs with both dtypes).
- ``round_to``: a float64 / float32 array rounded once to bf16 / fp16 by torch on the CPU, as float32 bits.
- ``half_ulp``: half a unit in the last place of the dtype at |ref|.
Test infrastructure only."""
from __future__ import annotations

import itertools

import numpy as np

DTYPES = ("bf16", "fp16")
DT_CODE = {"bf16": 1, "fp16": 2}              # NNC_DT_BF16, NNC_DT_F16 (include/nnc.h)
PATH_STREAM, PATH_MFMA = 1, 5                 # NNC_CBMM_STREAM, NNC_CBMM_MFMA
PRECISION = {"bf16": 8, "fp16": 11}           # significant bits
MIN_NORMAL_EXP = {"bf16": -126, "fp16": -14}

MS = (1, 2, 7, 16, 17, 33, 130)
KDIMS = (1, 3, 15, 17, 33, 100, 300, 1001)
NCOLS = (1, 16, 50, 129, 200)
MUST_SPLIT_KDIMS = (300, 1001)                # at every m of MS, on any device of 80 CUs or more


def torch_dtype(name):
    import torch

    return {"bf16": torch.bfloat16, "fp16": torch.float16}[name]


def _cases():
    cases = []
    i = 0
    for m, kdim in itertools.product(MS, KDIMS):
        lb = 1 + (i + i // 2) % 2
        k = (256, 17, 200)[i % 3] if lb == 1 else (257, 300, 1040, 17)[i % 4]
        cases.append(dict(m=m, kdim=kdim, ncols=NCOLS[i % len(NCOLS)], lb=lb, k=k, off=(0, 1, 3, 0, 5)[i % 5], x_view=i % 2 == 1,
                          bias=i % 4 != 2, bias_view=i % 3 == 1))
        i += 1
    return cases


CASES = _cases()


def case_id(c):
    return f"m{c['m']}-kd{c['kdim']}-n{c['ncols']}-lb{c['lb']}-k{c['k']}-o{c['off']}"


def regime_of(case, plan, dtype):
    assert plan["path"] in (PATH_STREAM, PATH_MFMA), plan
    return ("stream" if plan["path"] == PATH_STREAM else "mfma", case["lb"], "split" if plan["splits"] > 1 else "direct", dtype)


def required_regimes():
    return set(itertools.product(("stream", "mfma"), (1, 2), ("direct", "split"), DTYPES))


def round_to(values, dtype):
    """values rounded once (to nearest even, as torch.Tensor.to) to bf16 / fp16, returned as float32."""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32))
    return t.to(torch_dtype(dtype)).to(torch.float32).numpy()


def half_ulp(ref, dtype):
    """Half a unit in the last place of ``dtype`` at |ref| (float64): 2^(e - p) with e = floor(log2 |ref|) clamped to the least
    normal exponent (below it the spacing is the subnormal one: 2^-25 for fp16) and p the significant bits."""
    a = np.abs(np.asarray(ref, dtype=np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.maximum(np.where(a > 0, e, MIN_NORMAL_EXP[dtype]), MIN_NORMAL_EXP[dtype])
    return np.ldexp(1.0, (e - PRECISION[dtype]).astype(np.int64))
