"""Times the group-wise codebook backward pass on bfloat16 / float16 activations, byte and 4-bit packed indices
(ops.grouped_codebook_matmul_dx / _centroid_grad and the grouped_packed_* twins on half g and x: k_cbdx_mfma_grouped,
k_cbdc_mfma_grouped, k_cbpkdx_mfma_grouped, k_cbpkdc_mfma_grouped and the stream kernels) against (a) the
ungrouped half backward of this same build on the same indices with one table (ops.codebook_matmul_dx / _centroid_grad,
ops.packed_codebook_*) and (b) the float32 grouped kernels of this same build, one JSON line per (group_rows, m, dtype, state).

    python tools/time_grouped_codebook_backward_h16.py [--out FILE] [--quick]

The method of tools/time_codebook_backward_h16.py: each sequence of calls is captured in a HIP graph and replayed between HIP events
for at least 0.2 s, warm (the same indices every call) and cold (a rotation over distinct index matrices spanning >= 1 GiB of byte
labels; the packed rotation holds the same number of matrices, half the bytes).  Every column of a line comes from the same run.
The target of section 26, set before the first run: at 4096 x 4096, K = 16, group_rows = 128, m = 512, bf16, cold, grouped dx + dc
<= 1.10 x the ungrouped half dx + dc, for the byte pair and for the 4-bit packed pair ("pair_vs_ungrouped", "packed_pair_vs_ungrouped").
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

KDIM = NCOLS = 4096
K = 16
GROUP_ROWS = (128, 32)
MS = [1, 16, 256, 512, 4096]
DTYPES = (("bf16", torch.bfloat16), ("fp16", torch.float16))


def run(out, quick: bool):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    kdim, ncols, k = KDIM, NCOLS, K
    n = kdim * ncols
    rot = max(1, min(MAX_ROT, math.ceil(COLD_SPAN / n)))
    lbuf, lviews = _views(n, rot, torch.uint8, n, dev)
    lbuf.random_(0, k)
    codes = [ops.pack_codes(v, kdim, ncols, k, 4) for v in lviews]
    for gr in (GROUP_ROWS[:1] if quick else GROUP_ROWS):
        centers = torch.randn(kdim // gr, k, device=dev) * 0.05
        c1 = centers[0].contiguous()
        for dname, tdt in (DTYPES[:1] if quick else DTYPES):
            for m in ([16, 512] if quick else MS):
                x32 = torch.rand(m, kdim, device=dev)
                g32 = torch.randn(m, ncols, device=dev) * 1e-2
                x, g = x32.to(tdt), g32.to(tdt)
                for state in ("warm", "cold"):
                    def timed(fn):
                        nv = 1 if state == "warm" else rot
                        calls = max(rot, 16) if state == "warm" else rot
                        return _time_graph([(lambda i=i: fn(i % nv)) for i in range(calls)])

                    t = {
                        "dx": timed(lambda i: ops.grouped_codebook_matmul_dx(g, lviews[i], centers, kdim, ncols, gr)),
                        "dc": timed(lambda i: ops.grouped_codebook_centroid_grad(x, g, lviews[i], k, kdim, ncols, gr)),
                        "ungrouped_dx": timed(lambda i: ops.codebook_matmul_dx(g, lviews[i], c1, kdim, ncols)),
                        "ungrouped_dc": timed(lambda i: ops.codebook_centroid_grad(x, g, lviews[i], k, kdim, ncols)),
                        "dx_fp32": timed(lambda i: ops.grouped_codebook_matmul_dx(g32, lviews[i], centers, kdim, ncols, gr)),
                        "dc_fp32": timed(lambda i: ops.grouped_codebook_centroid_grad(x32, g32, lviews[i], k, kdim, ncols, gr)),
                        "packed_dx": timed(lambda i: ops.grouped_packed_codebook_matmul_dx(g, codes[i], centers, gr)),
                        "packed_dc": timed(lambda i: ops.grouped_packed_codebook_centroid_grad(x, g, codes[i], gr)),
                        "packed_ungrouped_dx": timed(lambda i: ops.packed_codebook_matmul_dx(g, codes[i], c1)),
                        "packed_ungrouped_dc": timed(lambda i: ops.packed_codebook_centroid_grad(x, g, codes[i])),
                        "packed_dx_fp32": timed(lambda i: ops.grouped_packed_codebook_matmul_dx(g32, codes[i], centers, gr)),
                        "packed_dc_fp32": timed(lambda i: ops.grouped_packed_codebook_centroid_grad(x32, g32, codes[i], gr)),
                    }
                    rec = {"case": f"{kdim}x{ncols}", "kdim": kdim, "ncols": ncols, "k": k, "group_rows": gr, "m": m, "dtype": dname, "state": state,
                           **{f"{key}_us": round(v * 1e6, 3) for key, v in t.items()},
                           "dx_vs_ungrouped": round(t["dx"] / t["ungrouped_dx"], 3), "dc_vs_ungrouped": round(t["dc"] / t["ungrouped_dc"], 3),
                           "pair_vs_ungrouped": round((t["dx"] + t["dc"]) / (t["ungrouped_dx"] + t["ungrouped_dc"]), 3),
                           "packed_dx_vs_ungrouped": round(t["packed_dx"] / t["packed_ungrouped_dx"], 3),
                           "packed_dc_vs_ungrouped": round(t["packed_dc"] / t["packed_ungrouped_dc"], 3),
                           "packed_pair_vs_ungrouped": round((t["packed_dx"] + t["packed_dc"]) / (t["packed_ungrouped_dx"] + t["packed_ungrouped_dc"]), 3),
                           "pair_vs_fp32": round((t["dx_fp32"] + t["dc_fp32"]) / (t["dx"] + t["dc"]), 3),
                           "packed_pair_vs_fp32": round((t["packed_dx_fp32"] + t["packed_dc_fp32"]) / (t["packed_dx"] + t["packed_dc"]), 3),
                           "rotation_span_mib": round((1 if state == "warm" else rot) * n / 2 ** 20, 1)}
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    ap.add_argument("--quick", action="store_true", help="group_rows = 128, bf16, m = 16 and 512 only")
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
