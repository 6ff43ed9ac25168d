"""Times the codebook backward pass (ops.codebook_matmul_dx: k_cbdx_stream / k_cbdx_tiled / k_cbgrad_reduce;
ops.codebook_centroid_grad: k_cbgrad_absmax, k_cbdc_stream / k_cbdc_tiled, k_cbdc_finish) against torch's dense backward on the
decoded float32 W (g @ W.T, x.T @ g, then ops.centroid_gradient of that dW), one JSON line per (shape, label width, m,
implementation).

    python tools/time_codebook_backward.py [--out FILE] [--quick]

The method of tools/time_codebook_matmul.py: each sequence of calls is captured in a HIP graph and replayed between HIP events for
at least 0.2 s, cold (a rotation over distinct index / float32 matrices spanning >= 1 GiB, four times the Infinity Cache; capped at
1024 matrices for the small LeNet shapes).  ops.centroid_gradient reads max |dW| back to the host once per call, which a graph
cannot hold: the torch baseline is therefore timed as the captured g @ W.T and x.T @ g plus, separately, the uncaptured
centroid_gradient calls in a loop (reported as "torch_dense" = their sum, and each part).  The bound of each case is the larger of
FLOPs / 157.3 TF and bytes / 8 TB/s (bytes: the index stream plus x, g, dx for the codebook pass; W, dW written and read again and
the labels for torch).
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from neural_network_compression_amd import ops  # noqa: E402
from tools.time_codebook_matmul import COLD_SPAN, MAX_ROT, PEAK_TBS, PEAK_TF, _time_graph, _views  # noqa: E402

SHAPES = [("lenet300.dense1", 784, 300, 16), ("lenet300.dense2", 300, 100, 16), ("lenet300.out", 100, 10, 16),
          ("lenet5.conv2", 500, 50, 16), ("lenet5.dense", 2450, 256, 16), ("5000x5000", 5000, 5000, 256), ("5000x5000", 5000, 5000, 257)]
MS = [1, 16, 256, 4096]


def _time_loop(fn, n) -> float:
    for _ in range(2):
        fn(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 0
    while time.perf_counter() - t0 < 0.2:
        fn(reps % n)
        reps += 1
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def run(out, quick: bool):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    shapes = SHAPES[-2:] if quick else SHAPES
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
        for i in range(rot_f):
            fviews[i].copy_(ops.gather(centers, lviews[i % rot]))
        for m in MS:
            if quick and m not in (1, 16, 256):
                continue
            x = torch.rand(m, kdim, device=dev)
            g = torch.randn(m, ncols, device=dev) * 1e-2
            t_dx = _time_graph([(lambda i=i: ops.codebook_matmul_dx(g, lviews[i], centers, kdim, ncols)) for i in range(rot)])
            t_dc = _time_graph([(lambda i=i: ops.codebook_centroid_grad(x, g, lviews[i], k, kdim, ncols)) for i in range(rot)])
            dxo = torch.empty(m, kdim, device=dev)
            dwo = torch.empty(kdim, ncols, device=dev)
            t_tdx = _time_graph([(lambda i=i: torch.matmul(g, fviews[i].view(kdim, ncols).t(), out=dxo)) for i in range(rot_f)])
            t_tdw = _time_graph([(lambda i=i: torch.matmul(x.t(), g, out=dwo)) for i in range(rot_f)])
            t_tcg = _time_loop(lambda i: ops.centroid_gradient(dwo, lviews[i % rot], k), rot)
            flops = 2.0 * m * kdim * ncols
            io = 4.0 * m * (2 * kdim + ncols)
            recs = [("codebook_dx", t_dx, n * lb + io, flops), ("codebook_dc", t_dc, n * lb + io, flops),
                    ("codebook_dx+dc", t_dx + t_dc, 2.0 * n * lb + 2 * io, 2 * flops),
                    ("torch_dx", t_tdx, n * 4.0 + io, flops), ("torch_dw", t_tdw, n * 4.0 + io, flops),
                    ("torch_centroid_gradient", t_tcg, n * (8.0 + lb), 0.0),
                    ("torch_dense", t_tdx + t_tdw + t_tcg, n * (16.0 + lb) + 2 * io, 2 * flops)]
            for impl, t, byts, fl in recs:
                t_min = max(fl / PEAK_TF, byts / PEAK_TBS)
                rec = {"case": name, "kdim": kdim, "ncols": ncols, "k": k, "label_bytes": lb, "m": m, "state": "cold", "impl": impl,
                       "us": round(t * 1e6, 3), "flops": fl, "bytes": byts, "tb_s": round(byts / t / 1e12, 3), "tflops": round(fl / t / 1e12, 3),
                       "bound": "compute" if fl / PEAK_TF >= byts / PEAK_TBS else "hbm", "share": round(t_min / t, 4),
                       "rotation_span_mib": round(rot * n * lb / 2 ** 20, 1)}
                if impl == "codebook_dx+dc":
                    rec["speedup_vs_torch_dense"] = round((t_tdx + t_tdw + t_tcg) / (t_dx + t_dc), 3)
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
            del dwo, dxo
        del lbuf, fbuf, lviews, fviews
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="the 5000 x 5000 shapes at m = 1, 16, 256 only")
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
