"""Times the codebook backward pass on bfloat16 / float16 activations (ops.codebook_matmul_dx / ops.codebook_centroid_grad on half g
and x: k_cbdx_stream<XT> / k_cbdx_mfma, k_cbdc_stream<XT> / k_cbdc_mfma) against (a) the float32 backward
pass of this same build on the same shapes and (b) torch's half backward on a decoded half W (g @ W.T, x.T @ g), one JSON line per
(shape, label width, m, dtype, state).

    python tools/time_codebook_backward_h16.py [--out FILE] [--quick]

The method of tools/time_codebook_matmul.py: each sequence of calls is captured in a HIP graph and replayed between HIP events for
at least 0.2 s, warm (the same indices every call) and cold (a rotation over distinct index / W matrices spanning >= 1 GiB, four
times the Infinity Cache).  Every column of a line comes from the same run.  The centroid sum behind torch's x.T @ g
(ops.centroid_gradient on the float32 dW) reads max |dW| back to the host, which a graph cannot hold: as in
tools/time_codebook_backward.py it is timed separately in an uncaptured loop and reported as its own column.
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
from tools.time_codebook_backward import _time_loop  # noqa: E402
from tools.time_codebook_matmul import COLD_SPAN, MAX_ROT, _time_graph, _views  # noqa: E402

SHAPES = [("4096x4096", 4096, 4096, 256), ("4096x4096", 4096, 4096, 257), ("5000x5000", 5000, 5000, 256), ("5000x5000", 5000, 5000, 257)]
MS = [1, 16, 256, 512, 4096]
DTYPES = (("bf16", torch.bfloat16), ("fp16", torch.float16))


def run(out, quick: bool):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    for name, kdim, ncols, k in (SHAPES[:1] if quick else SHAPES):
        lb = 1 if k <= 256 else 2
        n = kdim * ncols
        rot = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / (n * lb))))
        rot_h = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / (n * 2))))
        lbuf, lviews = _views(n * lb, rot, torch.uint8 if lb == 1 else torch.int16, n, dev)
        lbuf.random_(0, k)
        centers = torch.randn(k, device=dev) * 0.05
        t_tcg = None
        for dname, tdt in DTYPES:
            hbuf, hviews = _views(n * 2, rot_h, tdt, n, dev)
            for i in range(rot_h):
                hviews[i].copy_(ops.gather(centers, lviews[i % rot]).to(tdt))
            for m in ([16, 4096] if quick else MS):
                x32 = torch.rand(m, kdim, device=dev)
                g32 = torch.randn(m, ncols, device=dev) * 1e-2
                x, g = x32.to(tdt), g32.to(tdt)
                dxo = torch.empty(m, kdim, device=dev, dtype=tdt)
                dwo = torch.empty(kdim, ncols, device=dev, dtype=tdt)
                if t_tcg is None:
                    dw32 = torch.randn(kdim, ncols, device=dev)
                    t_tcg = _time_loop(lambda i: ops.centroid_gradient(dw32, lviews[i % rot], k), rot)
                    del dw32
                for state in ("warm", "cold"):
                    def timed(fn, count):
                        nv = 1 if state == "warm" else count
                        calls = max(count, 16) if state == "warm" else count
                        return _time_graph([(lambda i=i: fn(i % nv)) for i in range(calls)])

                    t = {
                        "dx": timed(lambda i: ops.codebook_matmul_dx(g, lviews[i], centers, kdim, ncols), rot),
                        "dc": timed(lambda i: ops.codebook_centroid_grad(x, g, lviews[i], k, kdim, ncols), rot),
                        "dx_fp32": timed(lambda i: ops.codebook_matmul_dx(g32, lviews[i], centers, kdim, ncols), rot),
                        "dc_fp32": timed(lambda i: ops.codebook_centroid_grad(x32, g32, lviews[i], k, kdim, ncols), rot),
                        "torch_dx": timed(lambda i: torch.matmul(g, hviews[i].view(kdim, ncols).t(), out=dxo), rot_h),
                        "torch_dw": timed(lambda i: torch.matmul(x.t(), g, out=dwo), rot_h),
                    }
                    flops = 2.0 * m * kdim * ncols
                    rec = {"case": name, "kdim": kdim, "ncols": ncols, "k": k, "label_bytes": lb, "m": m, "dtype": dname, "state": state,
                           **{f"{key}_us": round(v * 1e6, 3) for key, v in t.items()},
                           "torch_centroid_gradient_us": round(t_tcg * 1e6, 3),
                           "dx_tflops": round(flops / t["dx"] / 1e12, 2), "dc_tflops": round(flops / t["dc"] / 1e12, 2),
                           "dx_vs_fp32": round(t["dx_fp32"] / t["dx"], 3), "dc_vs_fp32": round(t["dc_fp32"] / t["dc"], 3),
                           "dx_vs_torch": round(t["torch_dx"] / t["dx"], 3), "dc_vs_torch_dw": round(t["torch_dw"] / t["dc"], 3),
                           "rotation_span_mib": round((1 if state == "warm" else rot) * n * lb / 2 ** 20, 1)}
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
                del dxo, dwo
            del hbuf, hviews
            torch.cuda.empty_cache()
        del lbuf, lviews
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="4096 x 4096, uint8, m = 16 and 4096 only")
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
