"""Times the codebook matmul (ops.codebook_matmul: k_cbmm_stream / k_cbmm_tiled / k_cbmm_reduce) against torch.matmul on the
decoded float32 weights, one JSON line per (shape, label width, m, cache state, implementation).

    python tools/time_codebook_matmul.py [--out FILE] [--quick]

Each measurement captures a sequence of calls in a HIP graph (torch.cuda.graph) and replays it with HIP events around the
replays, after a warm-up, for a window of at least 0.2 s: the time per call is then the device's, without the ~20 us of Python
per call that would otherwise hide a 5 us kernel.  States:
  warm  the same weights every call;
  cold  a rotation over distinct index (or float32) matrices spanning >= 1 GiB, four times the 256 MiB Infinity Cache (for the
        small LeNet shapes the rotation is capped at 1024 matrices and the span is reported).
The bound of each case is the larger of FLOPs / 157.3 TF and bytes / 8 TB/s (bytes: the weight stream -- indices for the
codebook matmul, float32 W for torch -- plus x and y); ``share`` is that least time over the measured time.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from neural_network_compression_amd import ops  # noqa: E402

PEAK_TF, PEAK_TBS = 157.3e12, 8.0e12
COLD_SPAN = 1 << 30
MAX_ROT = 1024
WINDOW_S = 0.2

SHAPES = [("lenet300.dense1", 784, 300, 16), ("lenet300.dense2", 300, 100, 16), ("lenet300.out", 100, 10, 16),
          ("lenet5.dense", 2450, 256, 16), ("4096x4096", 4096, 4096, 256), ("5000x5000", 5000, 5000, 256), ("5000x5000", 5000, 5000, 257)]
MS = [1, 4, 16, 256, 4096]


def _time_graph(fn_list) -> float:
    """Seconds per call of the captured sequence fn_list (each a no-argument callable)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for f in fn_list[: min(3, len(fn_list))]:
            f()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for f in fn_list:
            f()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    b.synchronize()
    once = max(a.elapsed_time(b) / 1e3, 1e-6)
    reps = max(1, math.ceil(WINDOW_S / once))
    a.record()
    for _ in range(reps):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 1e3 / (reps * len(fn_list))


def _views(nbytes_each: int, count: int, dtype, numel: int, dev):
    stride = (nbytes_each + 255) // 256 * 256
    esz = torch.tensor([], dtype=dtype).element_size()
    buf = torch.empty(stride * count // esz + numel, dtype=dtype, device=dev)
    return buf, [buf[i * stride // esz: i * stride // esz + numel] for i in range(count)]


def run(out, quick: bool):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    shapes = SHAPES[-3:] if quick else SHAPES
    for name, kdim, ncols, k in shapes:
        lb = 1 if k <= 256 else 2
        n = kdim * ncols
        rot = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / (n * lb))))
        rot_f = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / (n * 4))))
        ldt = torch.uint8 if lb == 1 else torch.int16
        lbuf, lviews = _views(n * lb, rot, ldt, n, dev)
        lbuf.random_(0, k)
        centers = torch.randn(k, device=dev) * 0.05
        fbuf, fviews = _views(n * 4, rot_f, torch.float32, n, dev)
        for i in range(rot_f):     # decoded W of the matching index matrix (the same values torch multiplies)
            fviews[i].copy_(ops.gather(centers, lviews[i % rot]))
        for m in MS:
            if quick and m not in (1, 16, 256):
                continue
            x = torch.rand(m, kdim, device=dev)
            flops = 2.0 * m * kdim * ncols
            io = 4.0 * m * (kdim + ncols)
            for state in ("warm", "cold"):
                nl = 1 if state == "warm" else rot
                nf = 1 if state == "warm" else rot_f
                calls = max(nl, 16) if state == "warm" else nl
                fns = [(lambda i=i: ops.codebook_matmul(x, lviews[i % nl], centers, kdim, ncols)) for i in range(calls)]
                t_cb = _time_graph(fns)
                yt = torch.empty(m, ncols, device=dev)
                calls_t = max(nf, 16) if state == "warm" else nf
                fnt = [(lambda i=i: torch.matmul(x, fviews[i % nf].view(kdim, ncols), out=yt)) for i in range(calls_t)]
                t_t = _time_graph(fnt)
                for impl, t, wbytes, span in (("codebook", t_cb, n * lb, nl * n * lb), ("torch_fp32", t_t, n * 4.0, nf * n * 4.0)):
                    byts = wbytes + io
                    t_min = max(flops / PEAK_TF, byts / PEAK_TBS)
                    rec = {"case": name, "kdim": kdim, "ncols": ncols, "k": k, "label_bytes": lb, "m": m, "state": state, "impl": impl,
                           "us": round(t * 1e6, 3), "flops": flops, "weight_bytes": wbytes, "bytes": byts,
                           "tb_s": round(byts / t / 1e12, 3), "weight_tb_s": round(wbytes / t / 1e12, 3), "tflops": round(flops / t / 1e12, 3),
                           "bound": "compute" if flops / PEAK_TF >= byts / PEAK_TBS else "hbm", "share": round(t_min / t, 4),
                           "rotation_span_mib": round(span / 2 ** 20, 1)}
                    if impl == "codebook":
                        rec["speedup_vs_torch"] = round(t_t / t_cb, 3)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
        del lbuf, fbuf, lviews, fviews
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="the 4096 / 5000 shapes at m = 1, 16, 256 only")
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
