"""Times the backward pass of the group-wise packed codebook matmul (ops.grouped_packed_codebook_matmul_dx /
grouped_packed_codebook_centroid_grad: csrc/nnc_cbpkgrad_grouped.hip) against its two yardsticks on the same
indices, one JSON line per (K, bits, group_rows, m, cache state, what, implementation).

    python tools/time_grouped_packed_codebook_backward.py [--out FILE] [--quick] [--step-timeout SECONDS]

4096 x 4096, K = 16 at 4 bits and K = 4 at 2 bits, group_rows = 128 and 32, m = 1, 16 and 256; ``what`` is dx or dc (float32
result).  The yardsticks are timed in the same run on the same indices, alternating with the code under test, which is never timed
alone: ops.packed_codebook_matmul_dx / ops.packed_codebook_centroid_grad with one table of K centres (``ungrouped_packed``), and
ops.grouped_codebook_matmul_dx / ops.grouped_codebook_centroid_grad on the uint8 labels (``grouped_byte``).  A ``grouped_packed``
row carries ``ratio`` (its time / the ungrouped packed call's) and ``vs_grouped_byte`` (the grouped byte call's time / its own).
Every figure is the median of REPEATS alternating rounds.  The method is tools/time_codebook_matmul.py's:
HIP events around replays of a captured graph, warm (the same indices every call) and cold (a rotation over distinct index
matrices spanning >= 1 GiB of the form that is read).

The parent process never opens the GPU: every (K, m) step runs in a child process of its own under ``--step-timeout``, and the
first step that fails or runs out of time ends the run (nothing more is started on the card).  The last line is the verdict on
the one target set before the first run: cold, group_rows = 128, m = 1 and m = 16, grouped packed at most 1.10 x ungrouped packed
for dx and dc at both widths."""
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
WIDTHS = ((16, 4), (4, 2))   # (K, bits)
GROUP_ROWS = (128, 32)
MS = (1, 16, 256)
REPEATS = 3
TARGET = 1.10      # group_rows = 128, m in (1, 16), cold, against the ungrouped packed calls


def step(k: int, m: int):
    """One child process: every row of (K, m), printed as JSON lines."""
    import torch

    from neural_network_compression_amd import ops
    from time_codebook_matmul import COLD_SPAN, MAX_ROT, _time_graph, _views

    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    bits = dict(WIDTHS)[k]
    n = KDIM * NCOLS
    cus = ops.device_info()[1]
    with torch.no_grad():
        rot_u = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / n)))
        lbuf, lviews = _views(n, rot_u, torch.uint8, n, dev)
        lbuf.random_(0, k)
        pbytes = ops.packed_nbytes(KDIM, NCOLS, bits)
        rot_p = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / pbytes)))
        codes = [ops.pack_codes(lviews[i % rot_u], KDIM, NCOLS, k, bits) for i in range(rot_p)]   # (codes[i] holds lviews[i % rot_u])
        flat = torch.randn(k, device=dev) * 0.05
        x = torch.rand(m, KDIM, device=dev)
        g = torch.randn(m, NCOLS, device=dev) * 1e-2
        for state in ("warm", "cold"):
            def timed(fn, rot):
                calls = max(rot, 16) if state == "warm" else rot
                nv = 1 if state == "warm" else rot
                return _time_graph([(lambda i=i: fn(i % nv)) for i in range(calls)])

            common = {"case": "4096x4096", "kdim": KDIM, "ncols": NCOLS, "k": k, "bits": bits, "m": m, "state": state}
            for rows in GROUP_ROWS:
                centers = (torch.randn(KDIM // rows, k, device=dev) * 0.05).contiguous()
                impls = {
                    ("ungrouped_packed", "dx"): (lambda i: ops.packed_codebook_matmul_dx(g, codes[i], flat), rot_p),
                    ("ungrouped_packed", "dc"): (lambda i: ops.packed_codebook_centroid_grad(x, g, codes[i], dtype=torch.float32), rot_p),
                    ("grouped_byte", "dx"): (lambda i: ops.grouped_codebook_matmul_dx(g, lviews[i], centers, KDIM, NCOLS, rows), rot_u),
                    ("grouped_byte", "dc"): (lambda i: ops.grouped_codebook_centroid_grad(x, g, lviews[i], k, KDIM, NCOLS, rows, dtype=torch.float32), rot_u),
                    ("grouped_packed", "dx"): (lambda i: ops.grouped_packed_codebook_matmul_dx(g, codes[i], centers, rows), rot_p),
                    ("grouped_packed", "dc"): (lambda i: ops.grouped_packed_codebook_centroid_grad(x, g, codes[i], rows, dtype=torch.float32), rot_p),
                }
                # the three implementations see the same matrix: the grouped dc is the grouped byte one bit for bit, its group sums
                # add up to the one-table sums
                assert torch.equal(impls[("grouped_packed", "dc")][0](0), impls[("grouped_byte", "dc")][0](0))
                one = impls[("ungrouped_packed", "dc")][0](0).double()
                assert torch.allclose(impls[("grouped_packed", "dc")][0](0).double().sum(0), one, rtol=1e-3, atol=1e-3 * float(one.abs().max()) + 1e-12)
                t = {key: [] for key in impls}
                for _ in range(REPEATS):                       # the yardsticks and the code under test alternate
                    for key, (fn, rot) in impls.items():
                        t[key].append(timed(fn, rot))
                med = {key: statistics.median(v) for key, v in t.items()}
                dxp = ops.cbpk_grouped_dx_plan(m, KDIM, NCOLS, bits, k, rows, cus)
                dcp = ops.cbpk_grouped_dc_plan(m, KDIM, NCOLS, bits, k, rows, cus)
                for (impl, what), sec in med.items():
                    rec = dict(common, impl=impl, what=what, group_rows=None if impl == "ungrouped_packed" else rows, us=round(sec * 1e6, 3),
                               repeats_us=[round(v * 1e6, 3) for v in t[(impl, what)]],
                               index_bytes=n if impl == "grouped_byte" else pbytes)
                    if impl == "grouped_packed":
                        plan = dxp if what == "dx" else dcp
                        rec.update(ratio=round(sec / med[("ungrouped_packed", what)], 4), vs_grouped_byte=round(med[("grouped_byte", what)] / sec, 3),
                                   path=plan["path"], vb=plan["vb"], splits=plan["splits"], rows_per_group=plan["rows_per_group"],
                                   max_groups_per_workgroup=plan["max_groups_per_workgroup"], held=plan["held"])
                    print(json.dumps(rec), flush=True)


def run(out, quick: bool, step_timeout: int):
    verdict = {}

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for k, bits in WIDTHS:
        for m in MS:
            if quick and m == 256:
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
                    if rec.get("impl") == "grouped_packed" and rec["group_rows"] == 128 and rec["state"] == "cold" and rec["m"] in (1, 16):
                        verdict[f"{rec['what']}-b{bits}-m{m}"] = rec["ratio"]
            if proc.returncode != 0:
                emit(json.dumps({"error": "step failed; nothing more is started", "step": [k, m], "returncode": proc.returncode,
                                 "stderr": proc.stderr[-2000:]}))
                return 1
    ok = bool(verdict) and all(v <= TARGET for v in verdict.values())
    emit(json.dumps({"target": "cold, group_rows = 128, m = 1 and m = 16: grouped packed <= 1.10 x ungrouped packed", "bound": TARGET,
                     "ratios": dict(sorted(verdict.items())), "verdict": "met" if ok else "missed", "worst": max(verdict.values()) if verdict else None}))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="m = 1 and m = 16 only (the rows of the target)")
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
