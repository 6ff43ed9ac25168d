"""Times the backward pass of the pruned group-wise codebook layer on bf16 activations from the bitmap-sparse form
(ops.grouped_sparse_codebook_matmul_dx / grouped_sparse_codebook_centroid_grad with half_inputs=True: csrc/nnc_cbspgrad_grouped_h16.hip,
DESIGN.md section 35) beside its ungrouped twin, the half sparse backward (nnc_cbsp_dx_h16 / nnc_cbsp_dc_h16) on the same buffer with
one codebook, one JSON line per (m, what, implementation).

    python tools/time_grouped_sparse_codebook_backward_h16.py [--out FILE] [--quick] [--step-timeout SECONDS]

4096 x 4096, K = 16, 10 % density, group_rows = 32 and 128, bfloat16, m = 4, 16 and 4096; ``what`` is dx (bfloat16 result) or dc
(float32 result).  Every group skips symbol 0, so the one buffer is also the ungrouped form's for zero_symbol = 0.  The method:
eager calls on one stream, HIP events around CALLS calls after a warm-up of every shape, ROUNDS rounds in which the ungrouped call and
the two grouped ones alternate in one process; a line carries the median of the rounds (``us`` per call), the spread (``min_us``,
``max_us``) and, for a grouped line, ``ratio`` = its median / the ungrouped median of the same rounds.  No graph is captured (the dc
entry points clear their workspace with a memset), so at m = 4 and 16 a call's time includes what the host needs to enqueue its
launches, the same for both implementations.

The parent process never opens the GPU: every m runs in a child process of its own under ``--step-timeout``, and the first step that
fails or runs out of time ends the run (nothing more is started on the card).  The last line states, row by row, whether the
project's customary target for a grouped variant is met: at most 1.10 x its ungrouped twin of the same run."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KDIM = NCOLS = 4096
K = 16
DENSITY = 0.1
GROUP_ROWS = (32, 128)
MS = (4, 16, 4096)
ROUNDS = 7
TARGET = 1.10      # against the ungrouped half sparse calls of the same run


def step(m: int):
    """One child process: every row of m, printed as JSON lines."""
    import torch

    from neural_network_compression_amd import ops

    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    n = KDIM * NCOLS
    calls = 2000 if m <= 16 else 100          # a timed window of 70 ms or more
    dt = torch.bfloat16
    with torch.no_grad():
        keep = torch.rand(n, device=dev) < DENSITY
        labels = torch.where(keep, torch.randint(1, K, (n,), device=dev), torch.zeros((), dtype=torch.int64, device=dev)).to(torch.uint8)
        del keep
        x = torch.rand(m, KDIM, device=dev).to(dt)
        g = (torch.randn(m, NCOLS, device=dev) * 1e-2).to(dt)
        flat = torch.randn(K, device=dev) * 0.05
        flat[0] = 0.0                                   # the pruned cluster: c_z == 0, as after prune -> quantize
        first = ops.pack_grouped_sparse_codes(labels, KDIM, NCOLS, K, GROUP_ROWS[0], zero_symbols=torch.zeros(KDIM // GROUP_ROWS[0], dtype=torch.uint8, device=dev))
        plain = ops.SparseCodes(first.buf, KDIM, NCOLS, K, 0, 1, first.nnz)
        impls = {"sparse_ungrouped_h16": {"dx": lambda: ops.sparse_codebook_matmul_dx(g, plain, flat),
                                          "dc": lambda: ops.sparse_codebook_centroid_grad(x, g, plain, dtype=torch.float32)}}
        for rows in GROUP_ROWS:
            G = KDIM // rows
            codes = ops.GroupedSparseCodes(first.buf, KDIM, NCOLS, K, rows, torch.zeros(G, dtype=torch.uint8, device=dev), first.nnz)
            centers = (torch.randn(G, K, device=dev) * 0.05).contiguous()
            centers[:, 0] = 0.0
            impls[f"sparse_grouped_h16_r{rows}"] = {
                "dx": lambda codes=codes, centers=centers: ops.grouped_sparse_codebook_matmul_dx(g, codes, centers, half_inputs=True),
                "dc": lambda codes=codes: ops.grouped_sparse_codebook_centroid_grad(x, g, codes, dtype=torch.float32, half_inputs=True)}
            # the groups' sums add up to the one-table sums (the same dW, the same shift)
            one = impls["sparse_ungrouped_h16"]["dc"]().double()
            assert torch.allclose(impls[f"sparse_grouped_h16_r{rows}"]["dc"]().double().sum(0), one, rtol=1e-3, atol=1e-3 * float(one.abs().max()) + 1e-12)

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3 / calls      # us per call

        for what in ("dx", "dc"):
            for fns in impls.values():                  # warm-up of every shape the timed window uses
                for _ in range(5):
                    fns[what]()
            torch.cuda.synchronize()
            times = {name: [] for name in impls}
            for _ in range(ROUNDS):                     # the implementations alternate
                for name, fns in impls.items():
                    times[name].append(timed(fns[what]))
            base = statistics.median(times["sparse_ungrouped_h16"])
            for name, ts in times.items():
                rec = {"case": "4096x4096", "k": K, "density": round(first.density(), 4), "dtype": "bf16", "m": m, "what": what, "impl": name,
                       "calls": calls, "rounds": ROUNDS, "us": round(statistics.median(ts), 3), "min_us": round(min(ts), 3), "max_us": round(max(ts), 3)}
                if name != "sparse_ungrouped_h16":
                    rec["ratio"] = round(statistics.median(ts) / base, 4)
                    rec["target_met"] = rec["ratio"] <= TARGET
                print(json.dumps(rec), flush=True)


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
                if "ratio" in rec:
                    verdict[f"{rec['what']}-{rec['impl'].rsplit('_', 1)[1]}-m{m}"] = rec["ratio"]
        if proc.returncode != 0:
            emit(json.dumps({"error": "step failed; nothing more is started", "step": m, "returncode": proc.returncode, "stderr": proc.stderr[-2000:]}))
            return 1
    missed = {k: v for k, v in verdict.items() if v > TARGET}
    emit(json.dumps({"target": "grouped sparse half backward <= 1.10 x the ungrouped half sparse backward of the same run, dx and dc separately",
                     "bound": TARGET, "ratios": dict(sorted(verdict.items())), "missed": dict(sorted(missed.items())),
                     "verdict": "met" if verdict and not missed else "missed", "worst": max(verdict.values()) if verdict else None}))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="m = 4 and m = 16 only")
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
