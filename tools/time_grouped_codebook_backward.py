"""Times the backward pass of the group-wise codebook matmul (ops.grouped_codebook_matmul_dx / grouped_codebook_centroid_grad:
csrc/nnc_cbgrad_grouped.hip) against the ungrouped calls on the same indices, one JSON line per (K,
group_rows, m, cache state, what, implementation).

    python tools/time_grouped_codebook_backward.py [--out FILE] [--quick] [--step-timeout SECONDS]

4096 x 4096, K = 16 and K = 256, group_rows = 128 and 32, m = 1, 16 and 256; ``what`` is dx, dc (float32 result) or dx + dc.  The
yardstick is timed in the same run on the same indices: ops.codebook_matmul_dx / ops.codebook_centroid_grad with one table of K
centres.  A grouped row carries ``ratio`` (its time / the yardstick's).  The method is tools/time_codebook_matmul.py's (DESIGN.md
section 10): HIP events around replays of a captured graph, warm (the same indices every call) and cold (a rotation over distinct
index matrices spanning >= 1 GiB).

The parent process never opens the GPU: every (K, m) step runs in a child process of its own under ``--step-timeout``, and the
first step that fails or runs out of time ends the run (nothing more is started on the card).  The last line is the verdict on
the one target set before the first run: cold, K = 16, group_rows = 128, m = 1 and m = 16, grouped at most 1.10 x ungrouped for
dx, dc and dx + dc."""
from __future__ import annotations

import argparse
import json
import math
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KDIM = NCOLS = 4096
KS = (16, 256)
GROUP_ROWS = (128, 32)
MS = (1, 16, 256)
TARGET = 1.10      # K = 16, group_rows = 128, m in (1, 16), cold, against the ungrouped calls


def step(k: int, m: int):
    """One child process: every row of (K, m), printed as JSON lines."""
    import torch

    from neural_network_compression_amd import ops
    from time_codebook_matmul import COLD_SPAN, MAX_ROT, _time_graph, _views

    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    n = KDIM * NCOLS
    cus = ops.device_info()[1]
    with torch.no_grad():
        rot = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / n)))
        lbuf, lviews = _views(n, rot, torch.uint8, n, dev)
        lbuf.random_(0, k)
        flat = torch.randn(k, device=dev) * 0.05
        x = torch.rand(m, KDIM, device=dev)
        g = torch.randn(m, NCOLS, device=dev) * 1e-2
        for state in ("warm", "cold"):
            def timed(fn):
                calls = max(rot, 16) if state == "warm" else rot
                nv = 1 if state == "warm" else rot
                return _time_graph([(lambda i=i: fn(i % nv)) for i in range(calls)])

            common = {"case": "4096x4096", "kdim": KDIM, "ncols": NCOLS, "k": k, "m": m, "state": state}
            plain = {
                "dx": lambda i: ops.codebook_matmul_dx(g, lviews[i], flat, KDIM, NCOLS),
                "dc": lambda i: ops.codebook_centroid_grad(x, g, lviews[i], k, KDIM, NCOLS, dtype=torch.float32),
            }
            plain["dx+dc"] = lambda i: (plain["dx"](i), plain["dc"](i))
            base = {}
            for what, fn in plain.items():
                base[what] = timed(fn)
                print(json.dumps(dict(common, impl="ungrouped", what=what, group_rows=None, us=round(base[what] * 1e6, 3),
                                      index_tb_s=round(n * (2 if what == "dx+dc" else 1) / base[what] / 1e12, 3))), flush=True)
            for rows in GROUP_ROWS:
                centers = (torch.randn(KDIM // rows, k, device=dev) * 0.05).contiguous()
                grouped = {
                    "dx": lambda i: ops.grouped_codebook_matmul_dx(g, lviews[i], centers, KDIM, NCOLS, rows),
                    "dc": lambda i: ops.grouped_codebook_centroid_grad(x, g, lviews[i], k, KDIM, NCOLS, rows, dtype=torch.float32),
                }
                grouped["dx+dc"] = lambda i: (grouped["dx"](i), grouped["dc"](i))
                # the grouped calls and the ungrouped ones bin the same dW: the group sums add up to the one-table sums
                one = plain["dc"](0).double()
                assert torch.allclose(grouped["dc"](0).double().sum(0), one, rtol=1e-3, atol=1e-3 * float(one.abs().max()) + 1e-12)
                dxp, dcp = ops.cbmm_grouped_dx_plan(m, KDIM, NCOLS, k, rows, cus), ops.cbmm_grouped_dc_plan(m, KDIM, NCOLS, k, rows, cus)
                for what, fn in grouped.items():
                    t = timed(fn)
                    print(json.dumps(dict(common, impl="grouped", what=what, group_rows=rows, us=round(t * 1e6, 3),
                                          index_tb_s=round(n * (2 if what == "dx+dc" else 1) / t / 1e12, 3), ratio=round(t / base[what], 4),
                                          path=dxp["path"], dx_splits=dxp["splits"], dc_splits=dcp["splits"], rows_per_group=dxp["rows_per_group"],
                                          max_groups_per_workgroup=dxp["max_groups_per_workgroup"])), flush=True)


def run(out, quick: bool, step_timeout: int):
    verdict = {}

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for k in KS:
        for m in MS:
            if quick and (m == 256 or k == 256):
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--step", f"{k},{m}"]
            try:
                proc = subprocess.run(cmd, capture_output=True, text=True, timeout=step_timeout)
            except subprocess.TimeoutExpired:
                emit(json.dumps({"error": "step ran out of time; nothing more is started", "step": [k, m], "timeout_s": step_timeout}))
                return 1
            for line in proc.stdout.splitlines():
                if line.startswith("{"):
                    emit(line)
                    rec = json.loads(line)
                    if rec.get("impl") == "grouped" and rec["k"] == 16 and rec["group_rows"] == 128 and rec["state"] == "cold" and rec["m"] in (1, 16):
                        verdict[f"{rec['what']}-m{m}"] = rec["ratio"]
            if proc.returncode != 0:
                emit(json.dumps({"error": "step failed; nothing more is started", "step": [k, m], "returncode": proc.returncode,
                                 "stderr": proc.stderr[-2000:]}))
                return 1
    ok = bool(verdict) and all(v <= TARGET for v in verdict.values())
    emit(json.dumps({"target": "cold, K = 16, group_rows = 128, m = 1 and m = 16: grouped <= 1.10 x ungrouped", "bound": TARGET,
                     "ratios": dict(sorted(verdict.items())), "verdict": "met" if ok else "missed", "worst": max(verdict.values()) if verdict else None}))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="K = 16 at m = 1 and m = 16 only (the rows of the target)")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds every child process may take")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)   # K,m: one child process
    a = ap.parse_args()
    if a.step:
        k, m = a.step.split(",")
        step(int(k), int(m))
        return 0
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            return run(f, a.quick, a.step_timeout)
    return run(None, a.quick, a.step_timeout)


if __name__ == "__main__":
    sys.exit(main())
