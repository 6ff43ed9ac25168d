"""Times the bitmap-sparse codebook matmul on bf16 / fp16 activations (ops.sparse_codebook_matmul on half x: k_cbsp_stream<half> /
k_cbsp_mfma / the split-K combines), one JSON line per (shape, density, m, cache state, implementation).

    python tools/time_sparse_codebook_matmul_h16.py [--out FILE] [--quick]

Each case is timed in the same run against (a) the float32 ops.sparse_codebook_matmul on the same form, (b) the byte form's half
path, ops.codebook_matmul on the unpacked indices and the same half x, and (c) torch.matmul(x_h, W.to(dtype)) on the decoded half W.
The method is tools/time_codebook_matmul_h16.py's: HIP events around replays of a captured graph, warm (the same weights every call)
and, up to 16 rows of x, cold (a rotation over distinct matrices spanning >= 1 GiB in each form).  The layers are 4096 x 4096 and
5000 x 5000, uint8 indices, K = 256, the skipped symbol 0 (centre 0, as after pruning) at densities 1, 10 and 32 %.  Implementations:
``sparse_bf16`` / ``sparse_fp16`` (half in, half out), ``sparse_fp32``, ``codebook_bf16`` / ``codebook_fp16``, ``torch_bf16`` /
``torch_fp16``.  ``weight_bytes`` is the resident form a call streams; the sparse half lines carry the ratios to (a), (b) and (c) as
``speedup_vs_sparse_fp32``, ``speedup_vs_codebook_half`` and ``speedup_vs_torch_half``.
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

SHAPES = [("4096x4096", 4096, 4096), ("5000x5000", 5000, 5000)]
K = 256
DENSITIES = [0.01, 0.10, 0.32]
MS = [1, 16, 256, 4096]
HALVES = (("bf16", torch.bfloat16), ("fp16", torch.float16))


def run(out, quick: bool):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    centers = torch.randn(K, device=dev) * 0.05
    centers[0] = 0.0
    for name, kdim, ncols in (SHAPES[1:] if quick else SHAPES):
        n = kdim * ncols
        rot = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / n)))
        rot_h = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / (n * 2))))
        for dens in ([0.10] if quick else DENSITIES):
            lbuf, lviews = _views(n, rot, torch.uint8, n, dev)
            for v in lviews:
                v.random_(1, K)
                v.masked_fill_(torch.rand(n, device=dev) >= dens, 0)
            sp0 = ops.pack_sparse_codes(lviews[0], kdim, ncols, K, zero_symbol=0)
            rot_s = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / sp0.nbytes())))
            codes = [sp0] + [ops.pack_sparse_codes(lviews[i % rot], kdim, ncols, K, zero_symbol=0) for i in range(1, rot_s)]
            hviews = {}
            for hname, hdt in HALVES:
                hbuf, hv = _views(n * 2, rot_h, hdt, n, dev)
                for i in range(rot_h):     # decoded half W of the matching index matrix (the values torch multiplies)
                    hv[i].copy_(ops.gather(centers, lviews[i % rot]))
                hviews[hname] = (hbuf, hv)
            for m in MS:
                if quick and m != 4096:
                    continue
                x = torch.rand(m, kdim, device=dev)
                flops = 2.0 * m * n
                for state in (("warm",) if m > 16 else ("warm", "cold")):
                    def timed(fn, count):
                        calls = max(count, 16) if state == "warm" else count
                        nv = 1 if state == "warm" else count
                        return _time_graph([(lambda i=i: fn(i % nv)) for i in range(calls)]), nv

                    res = {"sparse_fp32": timed(lambda i: ops.sparse_codebook_matmul(x, codes[i], centers), rot_s) + (sp0.nbytes(), 4)}
                    for hname, hdt in HALVES:
                        xh = x.to(hdt)
                        yh = torch.empty(m, ncols, device=dev, dtype=hdt)
                        hv = hviews[hname][1]
                        res["sparse_" + hname] = timed(lambda i: ops.sparse_codebook_matmul(xh, codes[i], centers), rot_s) + (sp0.nbytes(), 2)
                        res["codebook_" + hname] = timed(lambda i: ops.codebook_matmul(xh, lviews[i], centers, kdim, ncols), rot) + (n, 2)
                        res["torch_" + hname] = timed(lambda i: torch.matmul(xh, hv[i].view(kdim, ncols), out=yh), rot_h) + (n * 2, 2)
                    for impl, (t, nv, wbytes, esz) in res.items():
                        byts = wbytes + esz * m * (kdim + ncols)
                        rec = {"case": name, "kdim": kdim, "ncols": ncols, "k": K, "label_bytes": 1, "density": dens, "nnz": sp0.nnz, "m": m,
                               "state": state, "impl": impl, "us": round(t * 1e6, 3), "flops": flops, "weight_bytes": wbytes, "bytes": byts,
                               "tb_s": round(byts / t / 1e12, 3), "tflops": round(flops / t / 1e12, 3),
                               "rotation_span_mib": round(nv * wbytes / 2 ** 20, 1)}
                        if impl in ("sparse_bf16", "sparse_fp16"):
                            rec["speedup_vs_sparse_fp32"] = round(res["sparse_fp32"][0] / t, 3)
                            rec["speedup_vs_codebook_half"] = round(res["codebook_" + impl[-4:]][0] / t, 3)
                            rec["speedup_vs_torch_half"] = round(res["torch_" + impl[-4:]][0] / t, 3)
                        line = json.dumps(rec)
                        print(line, flush=True)
                        if out:
                            out.write(line + "\n")
                            out.flush()
            del lbuf, lviews, hviews, codes, sp0
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="5000 x 5000 at 10 %% density and m = 4096 only")
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
