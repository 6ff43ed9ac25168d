"""Times the group-wise packed codebook matmul (ops.grouped_packed_codebook_matmul: k_cbpk_stream_grouped / k_cbpk_mfma_grouped /
k_cbmm_reduce) against the ungrouped packed call and the byte-form grouped call on the same indices, one JSON
line per (K, bits, group_rows, m, dtype, cache state, implementation).

    python tools/time_grouped_packed_codebook_matmul.py [--out FILE] [--quick] [--step-timeout SECONDS]

4096 x 4096, K = 16 at 4 bits and K = 4 at 2 bits, group_rows = 128 and 32; m = 1 and m = 16 in float32, m = 4096 in bf16.  Two
yardsticks are timed in the same run on the same indices: ops.packed_codebook_matmul (the ungrouped packed call; float32 only, so
the bf16 rows have none) and ops.grouped_codebook_matmul on the uint8 labels.  A grouped packed row carries ``ratio_vs_packed``
and ``ratio_vs_byte_grouped`` (its time / the yardstick's).  The method is tools/time_codebook_matmul.py's: HIP events around
replays of a captured graph, warm (the same indices every call) and cold (a rotation over distinct index matrices spanning
>= 1 GiB of each form).

The parent process never opens the GPU: every (K, m) step runs in a child process of its own under ``--step-timeout``, and the
first step that fails or runs out of time ends the run (nothing more is started on the card).  The last line is the verdict on
the one target set before the first run: cold, group_rows = 128, m = 1 and m = 16, grouped packed at most 1.10 x ungrouped packed."""
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
WIDTHS = ((4, 16), (2, 4))                      # (bits, K)
GROUP_ROWS = (128, 32)
RUNS = ((1, "f32"), (16, "f32"), (4096, "bf16"))
TARGET = 1.10      # group_rows = 128, m in (1, 16), cold, against the ungrouped packed call


def step(bits: int, k: int, m: int, dname: str):
    """One child process: every row of (bits, K, m, dtype), printed as JSON lines."""
    import torch

    from neural_network_compression_amd import ops
    from time_codebook_matmul import COLD_SPAN, MAX_ROT, _time_graph, _views

    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    dt = {"f32": torch.float32, "bf16": torch.bfloat16}[dname]
    n = KDIM * NCOLS
    cus = ops.device_info()[1]
    with torch.no_grad():
        rot_u = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / n)))
        lbuf, lviews = _views(n, rot_u, torch.uint8, n, dev)
        lbuf.random_(0, k)
        pbytes = ops.packed_nbytes(KDIM, NCOLS, bits)
        rot_p = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / pbytes)))
        codes = [ops.pack_codes(lviews[i % rot_u], KDIM, NCOLS, k, bits) for i in range(rot_p)]
        flat = torch.randn(k, device=dev) * 0.05
        x = torch.rand(m, KDIM, device=dev).to(dt)
        for state in ("warm", "cold"):
            def timed(fn, rot):
                calls = max(rot, 16) if state == "warm" else rot
                nv = 1 if state == "warm" else rot
                return _time_graph([(lambda i=i: fn(i % nv)) for i in range(calls)])

            common = {"case": "4096x4096", "kdim": KDIM, "ncols": NCOLS, "k": k, "bits": bits, "m": m, "dtype": dname, "state": state}
            base = None
            if dt == torch.float32:
                base = timed(lambda i: ops.packed_codebook_matmul(x, codes[i], flat), rot_p)
                print(json.dumps(dict(common, impl="packed", group_rows=None, us=round(base * 1e6, 3), index_tb_s=round(pbytes / base / 1e12, 3))), flush=True)
            for rows in GROUP_ROWS:
                centers = (torch.randn(KDIM // rows, k, device=dev) * 0.05).contiguous()
                chk = torch.rand(3, KDIM, device=dev).to(dt)        # the two grouped forms multiply the same matrix
                assert torch.allclose(ops.grouped_packed_codebook_matmul(chk, codes[0], centers, rows).float(),
                                      ops.grouped_codebook_matmul(chk, lviews[0], centers, KDIM, NCOLS, rows).float(), rtol=2e-2, atol=2e-2)
                byte = timed(lambda i: ops.grouped_codebook_matmul(x, lviews[i], centers, KDIM, NCOLS, rows), rot_u)
                print(json.dumps(dict(common, impl="byte_grouped", group_rows=rows, us=round(byte * 1e6, 3), index_tb_s=round(n / byte / 1e12, 3))), flush=True)
                plan = ops.cbpk_grouped_plan(dt, m, KDIM, NCOLS, bits, k, rows, cus)
                t = timed(lambda i: ops.grouped_packed_codebook_matmul(x, codes[i], centers, rows), rot_p)
                print(json.dumps(dict(common, impl="grouped_packed", group_rows=rows, us=round(t * 1e6, 3), index_tb_s=round(pbytes / t / 1e12, 3),
                                      ratio_vs_packed=None if base is None else round(t / base, 4), ratio_vs_byte_grouped=round(t / byte, 4),
                                      path=plan["path"], vb=plan["vb"], mt=plan["mt"], splits=plan["splits"], rps=plan["rps"],
                                      max_groups_per_split=plan["max_groups_per_split"])), flush=True)


def run(out, quick: bool, step_timeout: int):
    verdict = {}

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for bits, k in WIDTHS:
        for m, dname in RUNS:
            if quick and m == 4096:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--step", f"{bits},{k},{m},{dname}"]
            try:
                proc = subprocess.run(cmd, capture_output=True, text=True, timeout=step_timeout)
            except subprocess.TimeoutExpired:
                emit(json.dumps({"error": "step ran out of time; nothing more is started", "step": [bits, k, m, dname], "timeout_s": step_timeout}))
                return 1
            for line in proc.stdout.splitlines():
                if line.startswith("{"):
                    emit(line)
                    rec = json.loads(line)
                    if rec.get("impl") == "grouped_packed" and rec["group_rows"] == 128 and rec["state"] == "cold" and rec["ratio_vs_packed"] is not None:
                        verdict[f"k{k}-m{m}"] = rec["ratio_vs_packed"]
            if proc.returncode != 0:
                emit(json.dumps({"error": "step failed; nothing more is started", "step": [bits, k, m, dname], "returncode": proc.returncode,
                                 "stderr": proc.stderr[-2000:]}))
                return 1
    ok = bool(verdict) and all(v <= TARGET for v in verdict.values())
    emit(json.dumps({"target": "cold, group_rows = 128, m = 1 and m = 16: grouped packed <= 1.10 x ungrouped packed", "bound": TARGET,
                     "ratios": dict(sorted(verdict.items())), "verdict": "met" if ok else "missed", "worst": max(verdict.values()) if verdict else None}))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="without the m = 4096 bf16 rows")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds every child process may take")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)   # bits,K,m,dtype: one child process
    a = ap.parse_args()
    if a.step:
        bits, k, m, dname = a.step.split(",")
        step(int(bits), int(k), int(m), dname)
        return 0
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            return run(f, a.quick, a.step_timeout)
    return run(None, a.quick, a.step_timeout)


if __name__ == "__main__":
    sys.exit(main())
