"""Times the group-wise codebook matmul (ops.grouped_codebook_matmul: k_cbmm_stream_grouped / k_cbmm_mfma_grouped / k_cbmm_reduce,
DESIGN.md section 17) against the ungrouped ops.codebook_matmul on the same indices, one JSON line per (K, group_rows, m, dtype,
cache state, implementation).

    python tools/time_grouped_codebook_matmul.py [--out FILE] [--quick]

4096 x 4096, K = 16 and K = 256, group_rows = 128 and 32; m = 1 and m = 16 in float32, m = 4096 in bf16.  Every grouped row is
timed in the same run as the ungrouped call and carries ``ratio_vs_ungrouped`` (grouped time / ungrouped time).  The method is
tools/time_codebook_matmul.py's: HIP events around replays of a captured graph, warm (the same indices every call) and cold (a
rotation over distinct index matrices spanning >= 1 GiB).  The last line is the verdict on the one target set before the first
run: K = 16, group_rows = 128, m = 1 and m = 16, cold, grouped at most 1.10 x ungrouped."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from neural_network_compression_amd import ops  # noqa: E402
from time_codebook_matmul import COLD_SPAN, MAX_ROT, _time_graph, _views  # noqa: E402

KDIM = NCOLS = 4096
KS = (16, 256)
GROUP_ROWS = (128, 32)
RUNS = ((1, torch.float32), (16, torch.float32), (4096, torch.bfloat16))
TARGET = 1.10      # K = 16, group_rows = 128, m in (1, 16), cold


def run(out, quick: bool):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    n = KDIM * NCOLS
    rot = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / n)))
    lbuf, lviews = _views(n, rot, torch.uint8, n, dev)
    verdict = {}

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for k in KS:
        lbuf.random_(0, k)
        flat = torch.randn(k, device=dev) * 0.05
        for m, dt in RUNS:
            if quick and m == 4096:
                continue
            x = torch.rand(m, KDIM, device=dev).to(dt)
            dname = {torch.float32: "f32", torch.bfloat16: "bf16"}[dt]
            for state in ("warm", "cold"):
                def timed(fn):
                    calls = max(rot, 16) if state == "warm" else rot
                    nv = 1 if state == "warm" else rot
                    return _time_graph([(lambda i=i: fn(i % nv)) for i in range(calls)])

                base = timed(lambda i: ops.codebook_matmul(x, lviews[i], flat, KDIM, NCOLS))
                common = {"case": "4096x4096", "kdim": KDIM, "ncols": NCOLS, "k": k, "m": m, "dtype": dname, "state": state}
                emit(dict(common, impl="ungrouped", group_rows=None, us=round(base * 1e6, 3), weight_tb_s=round(n / base / 1e12, 3)))
                for rows in GROUP_ROWS:
                    centers = (torch.randn(KDIM // rows, k, device=dev) * 0.05).contiguous()
                    plan = ops.cbmm_grouped_plan(dt, m, KDIM, NCOLS, k, rows, ops.device_info()[1])
                    t = timed(lambda i: ops.grouped_codebook_matmul(x, lviews[i], centers, KDIM, NCOLS, rows))
                    emit(dict(common, impl="grouped", group_rows=rows, us=round(t * 1e6, 3), weight_tb_s=round(n / t / 1e12, 3),
                              ratio_vs_ungrouped=round(t / base, 4), splits=plan["splits"], rps=plan["rps"],
                              max_groups_per_split=plan["max_groups_per_split"]))
                    if k == 16 and rows == 128 and m in (1, 16) and state == "cold":
                        verdict[m] = round(t / base, 4)
    ok = all(v <= TARGET for v in verdict.values())
    emit({"target": "K = 16, group_rows = 128, m = 1 and m = 16, cold: grouped <= 1.10 x ungrouped", "bound": TARGET,
          "ratios": {f"m{m}": v for m, v in sorted(verdict.items())}, "verdict": "met" if ok else "missed",
          "worst": max(verdict.values()) if verdict else None})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="without the m = 4096 bf16 rows")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    with torch.no_grad():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                run(f, a.quick)
        else:
            run(None, a.quick)


if __name__ == "__main__":
    main()
