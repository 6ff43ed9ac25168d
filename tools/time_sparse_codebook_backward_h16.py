"""Times the backward pass of the bitmap-sparse codebook layer on bfloat16 / float16 activations (ops.sparse_codebook_matmul_dx /
ops.sparse_codebook_centroid_grad on half g and x: k_cbspdx_stream<XT> / k_cbspdx_mfma, k_cbspdc_stream<XT> / k_cbspdc_mfma; DESIGN.md
section 24) against (a) the float32 sparse backward pass of this same build on the same form and (b) the byte form's half backward
pass on the unpacked labels, one JSON line per (shape, label width, density, m, dtype, state).

    python tools/time_sparse_codebook_backward_h16.py [--out FILE] [--quick]

The method of tools/time_codebook_backward_h16.py: each sequence of calls is captured in a HIP graph and replayed between HIP events
for at least 0.2 s, warm (the same form every call) and cold (a rotation over distinct copies of the form, or of the labels, spanning
>= 1 GiB, four times the Infinity Cache).  Every column of a line comes from the same run.
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
from tools.time_codebook_matmul import COLD_SPAN, MAX_ROT, _time_graph, _views  # noqa: E402
from tools.time_sparse_codebook_backward import _labels, _rotation  # noqa: E402

SHAPES = [("5000x5000", 5000, 5000, 256, 0.1), ("5000x5000", 5000, 5000, 256, 0.01), ("5000x5000", 5000, 5000, 256, 0.32),
          ("5000x5000", 5000, 5000, 257, 0.1)]
MS = [1, 16, 256, 512, 4096]
DTYPES = (("bf16", torch.bfloat16), ("fp16", torch.float16))


def run(out, quick: bool):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    for name, kdim, ncols, k, density in (SHAPES[:1] if quick else SHAPES):
        lb = 1 if k <= 256 else 2
        n = kdim * ncols
        labels = _labels(kdim, ncols, k, density, lb, dev)
        codes = ops.pack_sparse_codes(labels, kdim, ncols, k, zero_symbol=0)
        centers = torch.randn(k, device=dev) * 0.05
        rot_s = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / codes.nbytes())))
        rot_l = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / (n * lb))))
        srot = _rotation(codes, rot_s)
        lbuf, lviews = _views(n * lb, rot_l, labels.dtype, n, dev)
        for v in lviews:
            v.copy_(labels)
        for dname, tdt in (DTYPES[:1] if quick else DTYPES):
            for m in ([16, 4096] if quick else MS):
                x32 = torch.rand(m, kdim, device=dev)
                g32 = torch.randn(m, ncols, device=dev) * 1e-2
                x, g = x32.to(tdt), g32.to(tdt)
                for state in ("warm", "cold"):
                    def timed(fn, count):
                        nv = 1 if state == "warm" else count
                        calls = max(count, 16) if state == "warm" else count
                        return _time_graph([(lambda i=i: fn(i % nv)) for i in range(calls)])

                    t = {
                        "dx": timed(lambda i: ops.sparse_codebook_matmul_dx(g, srot[i], centers), rot_s),
                        "dc": timed(lambda i: ops.sparse_codebook_centroid_grad(x, g, srot[i]), rot_s),
                        "dx_fp32": timed(lambda i: ops.sparse_codebook_matmul_dx(g32, srot[i], centers), rot_s),
                        "dc_fp32": timed(lambda i: ops.sparse_codebook_centroid_grad(x32, g32, srot[i]), rot_s),
                        "byte_dx": timed(lambda i: ops.codebook_matmul_dx(g, lviews[i], centers, kdim, ncols), rot_l),
                        "byte_dc": timed(lambda i: ops.codebook_centroid_grad(x, g, lviews[i], k, kdim, ncols), rot_l),
                    }
                    flops = 2.0 * m * kdim * ncols
                    rec = {"case": name, "kdim": kdim, "ncols": ncols, "k": k, "label_bytes": lb, "density": round(codes.density(), 4), "m": m,
                           "dtype": dname, "state": state, **{f"{key}_us": round(v * 1e6, 3) for key, v in t.items()},
                           "dx_tflops": round(flops / t["dx"] / 1e12, 2), "dc_tflops": round(flops / t["dc"] / 1e12, 2),
                           "dx_vs_fp32": round(t["dx_fp32"] / t["dx"], 3), "dc_vs_fp32": round(t["dc_fp32"] / t["dc"], 3),
                           "dx+dc_vs_fp32": round((t["dx_fp32"] + t["dc_fp32"]) / (t["dx"] + t["dc"]), 3),
                           "dx_vs_byte": round(t["byte_dx"] / t["dx"], 3), "dc_vs_byte": round(t["byte_dc"] / t["dc"], 3),
                           "packed_bytes": codes.nbytes(), "rotation_span_mib": round((1 if state == "warm" else rot_s) * codes.nbytes() / 2 ** 20, 1)}
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
        del srot, lbuf, lviews, labels, codes
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="5000 x 5000, uint8, 10 %% density, bf16, m = 16 and 4096 only")
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
