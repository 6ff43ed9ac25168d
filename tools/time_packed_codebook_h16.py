"""Times the 2- / 4-bit packed codebook layer on bfloat16 / float16 activations (ops.packed_codebook_matmul / _matmul_dx /
_centroid_grad on half x and g: nnc_cbpk_h16, k_cbpkdx_stream<XT> / k_cbpkdx_mfma, k_cbpkdc_stream<XT> / k_cbpkdc_mfma; DESIGN.md
section 25) against (a) the float32 packed forward and backward of this same build on the same shapes and (b) the byte-form half
kernels on the unpacked labels (ops.codebook_matmul / codebook_matmul_dx / codebook_centroid_grad), one JSON line per (shape, bits, m,
dtype, state).

    python tools/time_packed_codebook_h16.py [--out FILE] [--quick] [--shape NAME]

The method of tools/time_codebook_matmul.py: each sequence of calls is captured in a HIP graph and replayed
between HIP events for at least 0.2 s, warm (the same indices every call) and cold (a rotation over distinct index matrices spanning
>= 1 GiB in each form, four times the Infinity Cache).  Every column of a line comes from the same run.
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

SHAPES = [("4096x4096", 4096, 4096), ("5000x5000", 5000, 5000)]
BITS = [(4, 16), (2, 4)]           # bits, K
MS = [1, 16, 256, 512, 4096]
DTYPES = (("bf16", torch.bfloat16), ("fp16", torch.float16))


def run(out, quick: bool, only: str | None):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    for name, kdim, ncols in SHAPES:
        if (quick and name != SHAPES[0][0]) or (only and name != only):
            continue
        n = kdim * ncols
        for bits, k in (BITS[:1] if quick else BITS):
            rot_b = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / n)))
            rot_p = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / ops.packed_nbytes(kdim, ncols, bits))))
            lbuf, lviews = _views(n, rot_b, torch.uint8, n, dev)
            lbuf.random_(0, k)
            codes = [ops.pack_codes(lviews[i % rot_b], kdim, ncols, k, bits) for i in range(rot_p)]
            centers = torch.randn(k, device=dev) * 0.05
            for dname, tdt in DTYPES:
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
                            "fwd": timed(lambda i: ops.packed_codebook_matmul(x, codes[i], centers), rot_p),
                            "dx": timed(lambda i: ops.packed_codebook_matmul_dx(g, codes[i], centers), rot_p),
                            "dc": timed(lambda i: ops.packed_codebook_centroid_grad(x, g, codes[i]), rot_p),
                            "fwd_fp32": timed(lambda i: ops.packed_codebook_matmul(x32, codes[i], centers), rot_p),
                            "dx_fp32": timed(lambda i: ops.packed_codebook_matmul_dx(g32, codes[i], centers), rot_p),
                            "dc_fp32": timed(lambda i: ops.packed_codebook_centroid_grad(x32, g32, codes[i]), rot_p),
                            "fwd_byte": timed(lambda i: ops.codebook_matmul(x, lviews[i], centers, kdim, ncols), rot_b),
                            "dx_byte": timed(lambda i: ops.codebook_matmul_dx(g, lviews[i], centers, kdim, ncols), rot_b),
                            "dc_byte": timed(lambda i: ops.codebook_centroid_grad(x, g, lviews[i], k, kdim, ncols), rot_b),
                        }
                        flops = 2.0 * m * kdim * ncols
                        rec = {"case": name, "kdim": kdim, "ncols": ncols, "bits": bits, "k": k, "m": m, "dtype": dname, "state": state,
                               **{f"{key}_us": round(v * 1e6, 3) for key, v in t.items()},
                               **{f"{d}_tflops": round(flops / t[d] / 1e12, 2) for d in ("fwd", "dx", "dc")},
                               **{f"{d}_vs_fp32": round(t[d + "_fp32"] / t[d], 3) for d in ("fwd", "dx", "dc")},
                               **{f"{d}_vs_byte": round(t[d + "_byte"] / t[d], 3) for d in ("fwd", "dx", "dc")},
                               "rotation_span_mib": round((1 if state == "warm" else rot_p) * codes[0].nbytes / 2 ** 20, 1)}
                        line = json.dumps(rec)
                        print(line, flush=True)
                        if out:
                            out.write(line + "\n")
                            out.flush()
            del lbuf, lviews, codes
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write (append) the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="4096 x 4096, 4 bits, m = 16 and 4096 only")
    ap.add_argument("--shape", default=None, help="only this shape (4096x4096 or 5000x5000)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    with torch.no_grad():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                run(f, a.quick, a.shape)
        else:
            run(None, a.quick, a.shape)


if __name__ == "__main__":
    main()
