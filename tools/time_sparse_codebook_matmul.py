"""Times the bitmap-sparse codebook matmul (ops.sparse_codebook_matmul: k_cbsp_stream / k_cbsp_tiled / k_cbsp_reduce) against
the dense codebook path (ops.codebook_matmul) and torch.matmul on the decoded float32 W, one JSON line per (density, m, cache
state, implementation).

    python tools/time_sparse_codebook_matmul.py [--out FILE] [--quick]

The method of tools/time_codebook_matmul.py: a sequence of calls captured in a HIP graph and replayed between HIP events for at
least 0.2 s.  warm: the same weights every call; cold: a rotation over distinct matrices spanning >= 1 GiB in each form (at
most 1024 of them; the span is reported).  The layer is 5000 x 5000, uint8 indices, K = 256, the skipped symbol 0 (centre 0,
as after pruning) at densities 1, 5, 10, 32 and 50 %.  ``weight_bytes`` is the resident form a call streams: the sparse
buffer, the dense indices, or the float32 W.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from neural_network_compression_amd import ops  # noqa: E402
from time_codebook_matmul import COLD_SPAN, MAX_ROT, PEAK_TBS, PEAK_TF, _time_graph, _views  # noqa: E402

KDIM = NCOLS = 5000
K = 256
DENSITIES = [0.01, 0.05, 0.10, 0.32, 0.50]
MS = [1, 16, 4096]


def run(out, quick: bool):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    n = KDIM * NCOLS
    rot = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / n)))
    rot_f = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / (n * 4))))
    centers = torch.randn(K, device=dev) * 0.05
    centers[0] = 0.0
    for dens in ([0.10, 0.32] if quick else DENSITIES):
        lbuf, lviews = _views(n, rot, torch.uint8, n, dev)
        for v in lviews:
            v.random_(1, K)
            v.masked_fill_(torch.rand(n, device=dev) >= dens, 0)
        sp0 = ops.pack_sparse_codes(lviews[0], KDIM, NCOLS, K, zero_symbol=0)
        rot_s = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / sp0.nbytes())))
        codes = [sp0] + [ops.pack_sparse_codes(lviews[i % rot], KDIM, NCOLS, K, zero_symbol=0) for i in range(1, rot_s)]
        fbuf, fviews = _views(n * 4, rot_f, torch.float32, n, dev)
        for i in range(rot_f):
            fviews[i].copy_(ops.gather(centers, lviews[i % rot]))
        for m in MS:
            if quick and m == 16:
                continue
            x = torch.rand(m, KDIM, device=dev)
            flops = 2.0 * m * n
            io = 4.0 * m * (KDIM + NCOLS)
            for state in (("warm",) if m > 16 else ("warm", "cold")):
                ns = 1 if state == "warm" else rot_s
                nl = 1 if state == "warm" else rot
                nf = 1 if state == "warm" else rot_f
                t_sp = _time_graph([(lambda i=i: ops.sparse_codebook_matmul(x, codes[i % ns], centers)) for i in range(max(ns, 16) if state == "warm" else ns)])
                t_cb = _time_graph([(lambda i=i: ops.codebook_matmul(x, lviews[i % nl], centers, KDIM, NCOLS)) for i in range(max(nl, 16) if state == "warm" else nl)])
                yt = torch.empty(m, NCOLS, device=dev)
                t_t = _time_graph([(lambda i=i: torch.matmul(x, fviews[i % nf].view(KDIM, NCOLS), out=yt)) for i in range(max(nf, 16) if state == "warm" else nf)])
                for impl, t, wbytes, span in (("sparse", t_sp, sp0.nbytes(), ns * sp0.nbytes()), ("codebook", t_cb, float(n), nl * float(n)),
                                              ("torch_fp32", t_t, 4.0 * n, nf * 4.0 * n)):
                    byts = wbytes + io
                    t_min = max(flops / PEAK_TF, byts / PEAK_TBS)
                    rec = {"case": f"{KDIM}x{NCOLS}", "kdim": KDIM, "ncols": NCOLS, "k": K, "label_bytes": 1, "density": dens,
                           "nnz": sp0.nnz, "m": m, "state": state, "impl": impl, "us": round(t * 1e6, 3), "weight_bytes": wbytes,
                           "bytes": byts, "tb_s": round(byts / t / 1e12, 3), "tflops": round(flops / t / 1e12, 3), "share": round(t_min / t, 4),
                           "rotation_span_mib": round(span / 2 ** 20, 1)}
                    if impl == "sparse":
                        rec["vs_codebook"] = round(t_sp / t_cb, 3)
                        rec["speedup_vs_torch"] = round(t_t / t_sp, 3)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
        del lbuf, lviews, fbuf, fviews, codes, sp0
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="densities 10 and 32 %% at m = 1 and 4096 only")
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
