"""Times the backward pass of the group-wise codebook layer on 5- and 6-bit split-plane indices (ops.grouped_wide_packed_codebook_matmul_dx /
ops.grouped_wide_packed_codebook_centroid_grad: the six kernels of csrc/nnc_cbwpgrad_grouped.hip) against two
yardsticks on the same labels, one JSON line per (K, bits, group_rows, m, dtype, direction, implementation).

    python tools/time_grouped_wide_packed_codebook_backward.py [--out FILE] [--quick] [--bits 5|6] [--step-timeout SECONDS]

4096 x 4096, K = 32 at 5 bits and K = 64 at 6 bits, group_rows = 32, 128 and 4096 (one group); m = 1 and 16 cold, m = 256 and 4096
warm, float32 and bf16.  The yardsticks, timed in the same child process on the same labels, are kernels this form's change does not
touch: (a) the group-wise byte backward on the uint8 labels (``byte_grouped``) and (b) the ungrouped split-plane backward of section
37 with one codebook (``wide_ungrouped``, which section 37 never timed; it does not depend on group_rows and is timed once per
step).  Each yardstick is timed three times: ``us`` is the median and ``range_us`` the range, the margin of the comparison.  A row of
the new form carries its ratio against each yardstick and met (not slower than the yardstick's median plus its range) or missed.

dx is timed as tools/time_codebook_matmul.py times a product: HIP events around replays of a captured graph.  dc clears its workspace
with a memset node, which is kept out of captured graphs here: it is timed eagerly, HIP events around a window of plain calls after a
warm-up, so at m <= 16 a dc row holds the wrapper's host time of either side as well.  Cold: a rotation over distinct index matrices
spanning >= 1 GiB of the byte form.  The parent process never opens the GPU: every (K, m, dtype) step runs in a child process of its
own under ``--step-timeout``, and the first step that fails or runs out of time ends the run (nothing more is started on the card)."""
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
GROUP_ROWS = (32, 128, KDIM)
RUNS = tuple((m, d, "cold" if m <= 16 else "warm") for d in ("f32", "bf16") for m in (1, 16, 256, 4096))
YARDSTICK_RUNS = 3
EAGER_WINDOW_S = 0.2


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

    def eager(fn, rot):
        """Seconds per call of fn(i), i rotating: a warm-up, one call to size the window, then events around the window."""
        for i in range(3):
            fn(i % rot)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn(0)
        b.record()
        b.synchronize()
        reps = max(rot, min(2000, math.ceil(EAGER_WINDOW_S / max(a.elapsed_time(b) / 1e3, 1e-6))))
        a.record()
        for i in range(reps):
            fn(i % rot)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / 1e3 / reps

    with torch.no_grad():
        rot = 1 if state == "warm" else max(1, min(MAX_ROT, math.ceil(COLD_SPAN / n)))
        lbuf, lviews = _views(n, rot, torch.uint8, n, dev)
        lbuf.random_(0, k)
        codes = [ops.pack_codes_wide(lviews[i], KDIM, NCOLS, k) for i in range(rot)]
        pbytes = codes[0].nbytes
        flat = torch.randn(k, device=dev) * 0.05
        x, g = torch.rand(m, KDIM, device=dev).to(dt), torch.randn(m, NCOLS, device=dev).to(dt)

        def timed(direction, fn):
            if direction == "dx":
                return _time_graph([(lambda i=i: fn(i % rot)) for i in range(max(rot, 16))])
            return eager(fn, rot)

        def yardstick(direction, fn):
            runs = [timed(direction, fn) for _ in range(YARDSTICK_RUNS)]
            return statistics.median(runs), max(runs) - min(runs)

        def verdict(t, ref):
            return "met" if t <= ref[0] + ref[1] else "missed"

        common = {"case": "4096x4096", "kdim": KDIM, "ncols": NCOLS, "k": k, "bits": bits, "m": m, "dtype": dname, "state": state}
        flat_calls = {"dx": lambda i: ops.wide_packed_codebook_matmul_dx(g, codes[i], flat),
                      "dc": lambda i: ops.wide_packed_codebook_centroid_grad(x, g, codes[i], dtype=torch.float32)}
        wide = {}
        for direction, fn in flat_calls.items():
            wide[direction] = yardstick(direction, fn)
            print(json.dumps(dict(common, impl="wide_ungrouped", direction=direction, group_rows=None, us=round(wide[direction][0] * 1e6, 3),
                                  range_us=round(wide[direction][1] * 1e6, 3))), flush=True)
        for rows in GROUP_ROWS:
            centers = (torch.randn(KDIM // rows, k, device=dev) * 0.05).contiguous()
            byte_calls = {"dx": lambda i: ops.grouped_codebook_matmul_dx(g, lviews[i], centers, KDIM, NCOLS, rows),
                          "dc": lambda i: ops.grouped_codebook_centroid_grad(x, g, lviews[i], k, KDIM, NCOLS, rows, dtype=torch.float32)}
            new_calls = {"dx": lambda i: ops.grouped_wide_packed_codebook_matmul_dx(g, codes[i], centers, rows),
                         "dc": lambda i: ops.grouped_wide_packed_codebook_centroid_grad(x, g, codes[i], rows, dtype=torch.float32)}
            assert torch.equal(new_calls["dc"](0), byte_calls["dc"](0))                       # the two grouped forms train the same matrix
            assert torch.allclose(new_calls["dx"](0).float(), byte_calls["dx"](0).float(), rtol=2e-2, atol=2e-2)
            plans = {"dx": ops.cbwp_grouped_dx_plan(dt, m, KDIM, NCOLS, bits, k, rows, cus), "dc": ops.cbwp_grouped_dc_plan(dt, m, KDIM, NCOLS, bits, k, rows, cus)}
            for direction in ("dx", "dc"):
                byte = yardstick(direction, byte_calls[direction])
                print(json.dumps(dict(common, impl="byte_grouped", direction=direction, group_rows=rows, us=round(byte[0] * 1e6, 3),
                                      range_us=round(byte[1] * 1e6, 3))), flush=True)
                t, p = timed(direction, new_calls[direction]), plans[direction]
                print(json.dumps(dict(common, impl="grouped_wide_packed", direction=direction, group_rows=rows, us=round(t * 1e6, 3),
                                      timing="graph" if direction == "dx" else "eager", index_tb_s=round(pbytes / t / 1e12, 3),
                                      ratio_vs_byte_grouped=round(t / byte[0], 4), vs_byte_grouped=verdict(t, byte),
                                      ratio_vs_wide_ungrouped=round(t / wide[direction][0], 4), vs_wide_ungrouped=verdict(t, wide[direction]),
                                      one_group=rows >= KDIM, path=p["path"], vb=p["vb"], mt=p["mt"], splits=p["splits"], held=p["held"],
                                      max_groups_per_workgroup=p["max_groups_per_workgroup"])), flush=True)


def run(out, quick: bool, step_timeout: int, only_bits=None):
    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for bits, k in WIDTHS:
        if only_bits not in (None, bits):
            continue
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
    ap.add_argument("--bits", type=int, choices=(5, 6), default=None, help="one width only (a run of its own per width halves the wall time of a call)")
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
            return run(f, a.quick, a.step_timeout, a.bits)
    return run(None, a.quick, a.step_timeout, a.bits)


if __name__ == "__main__":
    sys.exit(main())
