"""Times the group-wise codebook matmul on 5- and 6-bit split-plane indices (ops.grouped_wide_packed_codebook_matmul:
k_cbwp_stream_grouped / k_cbwp_tiled_grouped / k_cbwp_mfma_grouped / k_cbmm_reduce) against two yardsticks on the
same labels, one JSON line per (K, bits, group_rows, m, dtype, implementation).

    python tools/time_grouped_wide_packed_codebook_matmul.py [--out FILE] [--quick] [--step-timeout SECONDS]

4096 x 4096, K = 32 at 5 bits and K = 64 at 6 bits, group_rows = 128 and 32; m = 1 and m = 16 cold in float32, m = 256 and m = 4096
warm in float32 and bf16.  The yardsticks, timed in the same run on the same labels, are kernels this form's change does not touch:
ops.grouped_codebook_matmul on the uint8 labels (``byte_grouped``) and ops.wide_packed_codebook_matmul with one codebook
(``wide_ungrouped``).  Each yardstick is timed five times: ``us`` is the median and ``range_us`` the range of the five, the margin
of the comparison.  A row of the new form carries ``ratio_vs_byte_grouped`` and ``ratio_vs_wide_ungrouped`` and, against each, met
(not slower than the yardstick's median plus its range) or missed.  The bf16 steps at m = 256 and m = 4096 add a row with one group
(group_rows = kdim): the same grid and arithmetic as the ungrouped call, so its ratio against ``wide_ungrouped`` is the A/B of the
staged whole-word label decode against section 36's byte-per-row decode.  The expectation stated before any run: that ratio does not
show the 2.2 to 2.9 x that section 36 measured for the byte-per-row decode against the byte form.

The method is tools/time_codebook_matmul.py's: HIP events around replays of a captured graph, warm (the same indices every call)
or cold (a rotation over distinct index matrices spanning >= 1 GiB of each form).  The parent process never opens the GPU: every
(K, m, dtype) step runs in a child process of its own under ``--step-timeout``, and the first step that fails or runs out of time
ends the run (nothing more is started on the card)."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

KDIM = NCOLS = 4096
WIDTHS = ((5, 32), (6, 64))                     # (bits, K)
GROUP_ROWS = (128, 32)
RUNS = ((1, "f32", "cold"), (16, "f32", "cold"), (256, "f32", "warm"), (4096, "f32", "warm"), (256, "bf16", "warm"), (4096, "bf16", "warm"))
YARDSTICK_RUNS = 5


def step(bits: int, k: int, m: int, dname: str, state: str):
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
        pbytes = ops.wide_packed_nbytes(KDIM, NCOLS, bits)
        rot_u = 1 if state == "warm" else max(1, min(MAX_ROT, math.ceil(COLD_SPAN / n)))
        rot_p = 1 if state == "warm" else max(1, min(MAX_ROT, math.ceil(COLD_SPAN / pbytes)))
        lbuf, lviews = _views(n, rot_u, torch.uint8, n, dev)
        lbuf.random_(0, k)
        codes = [ops.pack_codes_wide(lviews[i % rot_u], KDIM, NCOLS, k) for i in range(rot_p)]
        flat = torch.randn(k, device=dev) * 0.05
        x = torch.rand(m, KDIM, device=dev).to(dt)

        def timed(fn, rot):
            return _time_graph([(lambda i=i: fn(i % rot)) for i in range(max(rot, 16))])

        def yardstick(fn, rot):
            runs = [timed(fn, rot) for _ in range(YARDSTICK_RUNS)]
            return statistics.median(runs), max(runs) - min(runs)

        def verdict(t, med, rng):
            return "met" if t <= med + rng else "missed"

        common = {"case": "4096x4096", "kdim": KDIM, "ncols": NCOLS, "k": k, "bits": bits, "m": m, "dtype": dname, "state": state}
        wide, wide_rng = yardstick(lambda i: ops.wide_packed_codebook_matmul(x, codes[i], flat), rot_p)
        print(json.dumps(dict(common, impl="wide_ungrouped", group_rows=None, us=round(wide * 1e6, 3), range_us=round(wide_rng * 1e6, 3))), flush=True)
        rows_list = GROUP_ROWS + ((KDIM,) if dname == "bf16" else ())
        for rows in rows_list:
            centers = (torch.randn(KDIM // rows, k, device=dev) * 0.05).contiguous()
            chk = torch.rand(3, KDIM, device=dev).to(dt)        # the two grouped forms multiply the same matrix
            assert torch.allclose(ops.grouped_wide_packed_codebook_matmul(chk, codes[0], centers, rows).float(),
                                  ops.grouped_codebook_matmul(chk, lviews[0], centers, KDIM, NCOLS, rows).float(), rtol=2e-2, atol=2e-2)
            byte, byte_rng = yardstick(lambda i: ops.grouped_codebook_matmul(x, lviews[i], centers, KDIM, NCOLS, rows), rot_u)
            print(json.dumps(dict(common, impl="byte_grouped", group_rows=rows, us=round(byte * 1e6, 3), range_us=round(byte_rng * 1e6, 3))), flush=True)
            plan = ops.cbwp_grouped_plan(dt, m, KDIM, NCOLS, bits, k, rows, cus)
            t = timed(lambda i: ops.grouped_wide_packed_codebook_matmul(x, codes[i], centers, rows), rot_p)
            print(json.dumps(dict(common, impl="grouped_wide_packed", group_rows=rows, us=round(t * 1e6, 3), index_tb_s=round(pbytes / t / 1e12, 3),
                                  ratio_vs_byte_grouped=round(t / byte, 4), vs_byte_grouped=verdict(t, byte, byte_rng),
                                  ratio_vs_wide_ungrouped=round(t / wide, 4), vs_wide_ungrouped=verdict(t, wide, wide_rng),
                                  one_group=rows >= KDIM, path=plan["path"], vb=plan["vb"], mt=plan["mt"], splits=plan["splits"], rps=plan["rps"],
                                  max_groups_per_split=plan["max_groups_per_split"])), flush=True)


def run(out, quick: bool, step_timeout: int):
    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for bits, k in WIDTHS:
        for m, dname, state in RUNS:
            if quick and m == 4096:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--step", f"{bits},{k},{m},{dname},{state}"]
            try:
                proc = subprocess.run(cmd, capture_output=True, text=True, timeout=step_timeout)
            except subprocess.TimeoutExpired:
                emit(json.dumps({"error": "step ran out of time; nothing more is started", "step": [bits, k, m, dname], "timeout_s": step_timeout}))
                return 1
            for line in proc.stdout.splitlines():
                if line.startswith("{"):
                    emit(line)
            if proc.returncode != 0:
                emit(json.dumps({"error": "step failed; nothing more is started", "step": [bits, k, m, dname], "returncode": proc.returncode,
                                 "stderr": proc.stderr[-2000:]}))
                return 1
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="without the m = 4096 rows")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds every child process may take")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)   # bits,K,m,dtype,state: one child process
    a = ap.parse_args()
    if a.step:
        bits, k, m, dname, state = a.step.split(",")
        step(int(bits), int(k), int(m), dname, state)
        return 0
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            return run(f, a.quick, a.step_timeout)
    return run(None, a.quick, a.step_timeout)


if __name__ == "__main__":
    sys.exit(main())
