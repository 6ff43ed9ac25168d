"""Times the half-precision codebook matmul (ops.codebook_matmul on bf16 / fp16 x: k_cbmm_stream<half> / k_cbmm_mfma /
k_cbmm_reduce), one JSON line per (shape, label width, m, cache state, implementation).

    python tools/time_codebook_matmul_h16.py [--out FILE] [--quick]

Each case is timed in the same run against (a) torch.matmul(x_h, W.to(dtype)) on the decoded half W, (b) the float32
ops.codebook_matmul on the same indices and (c) torch.matmul on the decoded float32 W.  The method is
tools/time_codebook_matmul.py's: HIP events around replays of a captured graph, warm (the same weights every call) and cold (a
rotation over distinct index / W matrices spanning >= 1 GiB).  Implementations: ``codebook_bf16`` / ``codebook_fp16`` (half in,
half out), ``torch_bf16`` / ``torch_fp16``, ``codebook_fp32``, ``torch_fp32``.  ``bytes`` counts the weight stream of the
implementation plus x and y in its own element sizes; the codebook lines carry the ratios to (a), (b) and (c) as
``speedup_vs_torch_half``, ``speedup_vs_codebook_fp32`` and ``speedup_vs_torch_fp32``.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from neural_network_compression_amd import ops  # noqa: E402
from time_codebook_matmul import COLD_SPAN, MAX_ROT, _time_graph, _views  # noqa: E402

SHAPES = [("4096x4096", 4096, 4096, 256), ("4096x4096", 4096, 4096, 257), ("5000x5000", 5000, 5000, 256), ("5000x5000", 5000, 5000, 257)]
MS = [1, 16, 256, 4096]
HALVES = (("bf16", torch.bfloat16), ("fp16", torch.float16))


def run(out, quick: bool):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    for name, kdim, ncols, k in (SHAPES[:1] if quick else SHAPES):
        lb = 1 if k <= 256 else 2
        n = kdim * ncols
        rot = {esz: max(1, min(MAX_ROT, math.ceil(COLD_SPAN / (n * esz)))) for esz in (1, 2, 4)}
        ldt = torch.uint8 if lb == 1 else torch.int16
        lbuf, lviews = _views(n * lb, rot[lb], ldt, n, dev)
        lbuf.random_(0, k)
        centers = torch.randn(k, device=dev) * 0.05
        fbuf, fviews = _views(n * 4, rot[4], torch.float32, n, dev)
        for i in range(rot[4]):     # decoded W of the matching index matrix (the same values torch multiplies)
            fviews[i].copy_(ops.gather(centers, lviews[i % rot[lb]]))
        hviews = {}
        for hname, hdt in HALVES:
            hbuf, hv = _views(n * 2, rot[2], hdt, n, dev)
            for i in range(rot[2]):
                hv[i].copy_(ops.gather(centers, lviews[i % rot[lb]]))
            hviews[hname] = (hbuf, hv)
        for m in MS:
            if quick and m not in (16, 4096):
                continue
            x = torch.rand(m, kdim, device=dev)
            flops = 2.0 * m * kdim * ncols
            for state in ("warm", "cold"):
                def timed(fn, count):
                    calls = max(count, 16) if state == "warm" else count
                    nv = 1 if state == "warm" else count
                    return _time_graph([(lambda i=i: fn(i % nv)) for i in range(calls)]), nv

                res = {}
                res["codebook_fp32"] = timed(lambda i: ops.codebook_matmul(x, lviews[i], centers, kdim, ncols), rot[lb]) + (n * lb, 4)
                yt = torch.empty(m, ncols, device=dev)
                res["torch_fp32"] = timed(lambda i: torch.matmul(x, fviews[i].view(kdim, ncols), out=yt), rot[4]) + (n * 4, 4)
                for hname, hdt in HALVES:
                    xh = x.to(hdt)
                    yh = torch.empty(m, ncols, device=dev, dtype=hdt)
                    hv = hviews[hname][1]
                    res["codebook_" + hname] = timed(lambda i: ops.codebook_matmul(xh, lviews[i], centers, kdim, ncols), rot[lb]) + (n * lb, 2)
                    res["torch_" + hname] = timed(lambda i: torch.matmul(xh, hv[i].view(kdim, ncols), out=yh), rot[2]) + (n * 2, 2)
                for impl, (t, nv, wbytes, esz) in res.items():
                    byts = wbytes + esz * m * (kdim + ncols)
                    rec = {"case": name, "kdim": kdim, "ncols": ncols, "k": k, "label_bytes": lb, "m": m, "state": state, "impl": impl,
                           "us": round(t * 1e6, 3), "flops": flops, "weight_bytes": wbytes, "bytes": byts, "tb_s": round(byts / t / 1e12, 3),
                           "weight_tb_s": round(wbytes / t / 1e12, 3), "tflops": round(flops / t / 1e12, 3),
                           "rotation_span_mib": round(nv * wbytes / 2 ** 20, 1)}
                    if impl in ("codebook_bf16", "codebook_fp16"):
                        rec["speedup_vs_torch_half"] = round(res["torch_" + impl[-4:]][0] / t, 3)
                        rec["speedup_vs_codebook_fp32"] = round(res["codebook_fp32"][0] / t, 3)
                        rec["speedup_vs_torch_fp32"] = round(res["torch_fp32"][0] / t, 3)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
        del lbuf, fbuf, lviews, fviews, hviews
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="4096 x 4096 with uint8 indices at m = 16 and 4096 only")
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
