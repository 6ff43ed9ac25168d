"""Times the backward pass of the group-wise codebook layer from the bitmap-sparse form (ops.grouped_sparse_codebook_matmul_dx /
grouped_sparse_codebook_centroid_grad: csrc/nnc_cbspgrad_grouped.hip) beside the ungrouped sparse backward on
the same indices with one codebook and beside the grouped byte backward, one JSON line per (group_rows, m, cache state, what,
implementation).

    python tools/time_grouped_sparse_codebook_backward.py [--out FILE] [--quick] [--step-timeout SECONDS]

4096 x 4096, K = 16, 10 % density, group_rows = 128 and 32, m = 1, 16 and 4096; ``what`` is dx or dc (float32 result).  Every group
skips symbol 0, so the one buffer is also the ungrouped form's for zero_symbol = 0: the yardstick, ops.sparse_codebook_matmul_dx /
sparse_codebook_centroid_grad with one table of K centres, is timed in the same run on the same buffers; the grouped byte backward
(ops.grouped_codebook_matmul_dx / grouped_codebook_centroid_grad) runs on the unpacked labels.  A grouped sparse row carries ``ratio``
(its time / the ungrouped sparse call's) and ``vs_byte`` (its time / the grouped byte call's).  The method is
tools/time_codebook_matmul.py's: HIP events around replays of a captured graph, warm (the same buffer every
call) and cold (a rotation over distinct copies spanning >= 1 GiB; at m = 4096, where the index traffic is a small share of the
call, over at most 16 copies).

The parent process never opens the GPU: every m runs in a child process of its own under ``--step-timeout``, and the first step
that fails or runs out of time ends the run (nothing more is started on the card).  The last line is the verdict on the target set
before the first run: grouped sparse at most 1.10 x the ungrouped sparse backward of the same run, dx and dc separately, row by row."""
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
K = 16
DENSITY = 0.1
GROUP_ROWS = (128, 32)
MS = (1, 16, 4096)
TARGET = 1.10      # against the ungrouped sparse calls of the same run


def step(m: int):
    """One child process: every row of m, printed as JSON lines."""
    import torch

    from neural_network_compression_amd import ops
    from time_codebook_matmul import COLD_SPAN, MAX_ROT, _time_graph, _views

    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    n = KDIM * NCOLS
    cus = ops.device_info()[1]
    with torch.no_grad():
        keep = torch.rand(n, device=dev) < DENSITY
        labels = torch.where(keep, torch.randint(1, K, (n,), device=dev), torch.zeros((), dtype=torch.int64, device=dev)).to(torch.uint8)
        del keep
        cap = MAX_ROT if m <= 256 else 16
        x = torch.rand(m, KDIM, device=dev)
        g = torch.randn(m, NCOLS, device=dev) * 1e-2
        flat = torch.randn(K, device=dev) * 0.05
        flat[0] = 0.0                                   # the pruned cluster: c_z == 0, as after prune -> quantize
        first = ops.pack_grouped_sparse_codes(labels, KDIM, NCOLS, K, GROUP_ROWS[0],
                                              zero_symbols=torch.zeros(KDIM // GROUP_ROWS[0], dtype=torch.uint8, device=dev))
        rot_s = max(1, min(cap, math.ceil(COLD_SPAN / first.buf.numel())))
        rot_l = max(1, min(cap, math.ceil(COLD_SPAN / n)))
        bufs = []
        for _ in range(rot_s):
            b = ops._aligned_bytes(first.buf.numel(), dev)
            b.copy_(first.buf)
            bufs.append(b)
        lbuf, lviews = _views(n, rot_l, torch.uint8, n, dev)
        for v in lviews:
            v.copy_(labels)
        del labels
        plain_codes = [ops.SparseCodes(b, KDIM, NCOLS, K, 0, 1, first.nnz) for b in bufs]
        for state in ("warm", "cold"):
            def timed(fn, rot):
                calls = max(min(rot, 16), 4) if state == "warm" else rot
                nv = 1 if state == "warm" else rot
                return _time_graph([(lambda i=i: fn(i % nv)) for i in range(calls)])

            common = {"case": "4096x4096", "kdim": KDIM, "ncols": NCOLS, "k": K, "density": round(first.density(), 4), "m": m, "state": state,
                      "packed_bytes": first.buf.numel()}
            plain = {"dx": lambda i: ops.sparse_codebook_matmul_dx(g, plain_codes[i], flat),
                     "dc": lambda i: ops.sparse_codebook_centroid_grad(x, g, plain_codes[i], dtype=torch.float32)}
            base = {}
            for what, fn in plain.items():
                base[what] = timed(fn, rot_s)
                print(json.dumps(dict(common, impl="sparse_ungrouped", what=what, group_rows=None, us=round(base[what] * 1e6, 3))), flush=True)
            for rows in GROUP_ROWS:
                G = KDIM // rows
                zs = torch.zeros(G, dtype=torch.uint8, device=dev)
                centers = (torch.randn(G, K, device=dev) * 0.05).contiguous()
                centers[:, 0] = 0.0
                gcodes = [ops.GroupedSparseCodes(b, KDIM, NCOLS, K, rows, zs, first.nnz) for b in bufs]
                sparse = {"dx": lambda i: ops.grouped_sparse_codebook_matmul_dx(g, gcodes[i], centers),
                          "dc": lambda i: ops.grouped_sparse_codebook_centroid_grad(x, g, gcodes[i], dtype=torch.float32)}
                byte = {"dx": lambda i: ops.grouped_codebook_matmul_dx(g, lviews[i], centers, KDIM, NCOLS, rows),
                        "dc": lambda i: ops.grouped_codebook_centroid_grad(x, g, lviews[i], K, KDIM, NCOLS, rows, dtype=torch.float32)}
                # the two grouped forms bin the same dW bit for bit, and the groups' sums add up to the one-table sums
                assert torch.equal(sparse["dc"](0), byte["dc"](0))
                one = plain["dc"](0).double()
                assert torch.allclose(sparse["dc"](0).double().sum(0), one, rtol=1e-3, atol=1e-3 * float(one.abs().max()) + 1e-12)
                dxp, dcp = ops.cbsp_grouped_dx_plan(m, KDIM, NCOLS, K, rows, cus), ops.cbsp_grouped_dc_plan(m, KDIM, NCOLS, K, rows, cus)
                for what in ("dx", "dc"):
                    tb = timed(byte[what], rot_l)
                    print(json.dumps(dict(common, impl="byte_grouped", what=what, group_rows=rows, us=round(tb * 1e6, 3))), flush=True)
                    t = timed(sparse[what], rot_s)
                    p = dxp if what == "dx" else dcp
                    print(json.dumps(dict(common, impl="sparse_grouped", what=what, group_rows=rows, us=round(t * 1e6, 3), ratio=round(t / base[what], 4),
                                          vs_byte=round(t / tb, 4), path=p["path"], splits=p["splits"], rows_per_group=p["rows_per_group"],
                                          max_groups_per_workgroup=p["max_groups_per_workgroup"])), flush=True)


def run(out, quick: bool, step_timeout: int):
    verdict = {}

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for m in MS:
        if quick and m > 16:
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(m)]
        try:
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=step_timeout)
        except subprocess.TimeoutExpired:
            emit(json.dumps({"error": "step ran out of time; nothing more is started", "step": m, "timeout_s": step_timeout}))
            return 1
        for line in proc.stdout.splitlines():
            if line.startswith("{"):
                emit(line)
                rec = json.loads(line)
                if rec.get("impl") == "sparse_grouped":
                    verdict[f"{rec['what']}-r{rec['group_rows']}-m{m}-{rec['state']}"] = rec["ratio"]
        if proc.returncode != 0:
            emit(json.dumps({"error": "step failed; nothing more is started", "step": m, "returncode": proc.returncode, "stderr": proc.stderr[-2000:]}))
            return 1
    missed = {k: v for k, v in verdict.items() if v > TARGET}
    emit(json.dumps({"target": "grouped sparse <= 1.10 x the ungrouped sparse backward of the same run, dx and dc separately", "bound": TARGET,
                     "ratios": dict(sorted(verdict.items())), "missed": dict(sorted(missed.items())),
                     "verdict": "met" if verdict and not missed else "missed", "worst": max(verdict.values()) if verdict else None}))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="m = 1 and m = 16 only")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds every child process may take")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)   # m: one child process
    a = ap.parse_args()
    if a.step:
        step(int(a.step))
        return 0
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            return run(f, a.quick, a.step_timeout)
    return run(None, a.quick, a.step_timeout)


if __name__ == "__main__":
    sys.exit(main())
